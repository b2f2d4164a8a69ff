"""Activation checkpointing of the SwAV trunk (ResNet50Trunk(checkpoint_stages=True)) on the CPU
reference operators: layer1-layer3 run as replayed segments whose recompute applies the first pass's
saved BatchNorm statistics, so the result is the plain trunk's — counters, running statistics,
output and every gradient.

The comparisons are exact.  The CPU operators are deterministic on one thread (the max-pool backward
is an overwriting scatter over overlapping windows, whose winner depends on the thread schedule), so
every test here runs single-threaded."""
import logging
import math

import pytest
import torch

from dedloc_amd.utils.config import load_config
from dedloc_amd.models.resnet_swav import BNAct, ResNet50Trunk, SwAVModel

CL = torch.channels_last


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _img(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g).to(torch.bfloat16).contiguous(memory_format=CL)


def _twins(make):
    """(checkpointed, plain) with equal parameters and buffers, in training mode."""
    torch.manual_seed(0)
    a, b = make(True), make(False)
    b.load_state_dict(a.state_dict())
    return a.train(), b.train()


def _assert_state_equal(a, b, what):
    for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), f"{what}: buffer {n}"
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is not None and q.grad is not None, f"{what}: no gradient for {n}"
        assert torch.equal(p.grad, q.grad), f"{what}: gradient of {n}"


def test_trunk_equals_plain_twin():
    """Three iterations: after each, every BN counter / running statistic, the output and every
    parameter gradient (accumulated over the iterations) equal the plain trunk's."""
    a, b = _twins(lambda ck: ResNet50Trunk(checkpoint_stages=ck))
    for it in range(3):
        x = _img(4, 32, 10 + it)
        ya, yb = a(x), b(x)
        dy = torch.randn(ya.shape, generator=torch.Generator().manual_seed(20 + it)).to(ya.dtype)
        ya.backward(dy)
        yb.backward(dy)
        assert torch.equal(ya, yb), f"iteration {it}: output"
        _assert_state_equal(a, b, f"iteration {it}")
        for m in a.modules():
            if isinstance(m, BNAct):
                assert int(m.num_batches_tracked) == it + 1


@pytest.mark.parametrize("single_pass_every_crop", [True, False])
def test_swav_model_equals_plain_twin(single_pass_every_crop):
    """The reference's configuration (per-crop statistics groups, two resolution passes): the
    recompute restores each call's own state, not what the last pass left in the modules."""
    a, b = _twins(lambda ck: SwAVModel(num_prototypes=16, single_pass_every_crop=single_pass_every_crop,
                                       checkpoint_stages=ck))
    crops = [_img(2, 32, 1), _img(2, 32, 2), _img(2, 16, 3), _img(2, 16, 4), _img(2, 16, 5)]
    (ea, sa), (eb, sb) = a(crops), b(crops)
    g = torch.Generator().manual_seed(6)
    de, ds = torch.randn(ea.shape, generator=g).to(ea.dtype), torch.randn(sa.shape, generator=g).to(sa.dtype)
    torch.autograd.backward([ea, sa], [de, ds])
    torch.autograd.backward([eb, sb], [de, ds])
    assert torch.equal(ea, eb) and torch.equal(sa, sb)
    _assert_state_equal(a, b, f"single_pass_every_crop={single_pass_every_crop}")


def _count(monkeypatch, names):
    calls = {n: 0 for n in names}
    for n in names:
        op = getattr(torch.ops.dedloc, n)

        def wrapped(*args, _op=op, _n=n, **kw):
            calls[_n] += 1
            return _op(*args, **kw)

        monkeypatch.setattr(torch.ops.dedloc, n, wrapped)
    return calls


def test_recompute_runs_no_statistics(monkeypatch):
    """During backward() no statistics are computed — neither bn_fwd nor a conv statistics epilogue
    runs (the stem and layer4 are not recomputed, so the whole backward makes zero such calls) — and
    bn_apply runs once per BatchNorm of layer1-layer3."""
    a, _ = _twins(lambda ck: ResNet50Trunk(checkpoint_stages=ck))
    n_replayed = sum(isinstance(m, BNAct) for s in (a.layer1, a.layer2, a.layer3) for m in s.modules())
    n_all = sum(isinstance(m, BNAct) for m in a.modules())
    assert n_replayed == 42 and n_all == 53
    calls = _count(monkeypatch, ["bn_fwd", "conv2d_fwd_stats", "bn_apply", "conv2d_fwd"])
    y = a(_img(4, 32, 1))
    # the first pass is today's: every BN from conv-epilogue statistics
    assert calls == {"bn_fwd": n_all, "conv2d_fwd_stats": n_all, "bn_apply": 0, "conv2d_fwd": 0}
    for k in calls:
        calls[k] = 0
    y.sum().backward()
    assert calls["bn_fwd"] == 0 and calls["conv2d_fwd_stats"] == 0
    assert calls["bn_apply"] == n_replayed and calls["conv2d_fwd"] == n_replayed


def test_plain_fallback_records_nothing(monkeypatch):
    """eval() and a no_grad forward run every stage plain: equal to the plain trunk, nothing recorded."""
    from dedloc_amd.models import resnet_swav

    a, b = _twins(lambda ck: ResNet50Trunk(checkpoint_stages=ck))
    made = []
    init = resnet_swav._SegmentRecord.__init__
    monkeypatch.setattr(resnet_swav._SegmentRecord, "__init__",
                        lambda self, mods: (made.append(self), init(self, mods))[1])
    x = _img(4, 32, 1)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), n
    a.eval()
    b.eval()
    assert torch.equal(a(x), b(x))
    assert not made
    # (an input that takes no gradient: the stem's output always does in training, so a frozen trunk)
    a.train()
    for p in a.parameters():
        p.requires_grad_(False)
    a(x)
    assert not made
    for p in a.parameters():
        p.requires_grad_(True)
    a(x)
    assert len(made) == 3  # layer1, layer2, layer3


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_apply_equals_bn_fwd_cpu(G, res, relu):
    g = torch.Generator().manual_seed(G)
    x = (torch.randn(6, 64, 5, 5, generator=g) * 2 + 0.5).to(torch.bfloat16).contiguous(memory_format=CL)
    r = torch.randn(6, 64, 5, 5, generator=g).to(torch.bfloat16).contiguous(memory_format=CL) if res else None
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    rm, rv = torch.zeros(64), torch.ones(64)
    y, mean, rstd = torch.ops.dedloc.bn_fwd(x, r, gamma, beta, rm, rv, 1e-5, 0.1, relu, G, None, False)
    rm0, rv0 = rm.clone(), rv.clone()
    y2 = torch.ops.dedloc.bn_apply(x, r, gamma, beta, mean, rstd, relu, G)
    assert y2.dtype == y.dtype and y2.is_contiguous(memory_format=CL)
    assert torch.equal(y2, y)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    # the given statistics are used, not re-derived from x
    y3 = torch.ops.dedloc.bn_apply(x, r, gamma, beta, mean + 1.0, rstd, relu, G)
    assert not torch.equal(y3, y)


def test_peer_steps_with_checkpointing(tmp_path, caplog):
    """A SwavPeer as in test_swav_peer_cpu_steps_and_checkpoint with the override on: two steps with
    a finite loss, and one log line that concurrent passes and graphs are off."""
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer

    cfg = load_config("swav_1node_resnet_submit", [
        "config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=2", "config.DATA.TRAIN.MULTICROP.size_crops=[32,16]",
        "config.DATA.TRAIN.MULTICROP.num_crops=[2,2]",
        "config.DATA.TRAIN.SYNTHETIC_POOL_SIZE=4", "config.DATA.TRAIN.SYNTHETIC_IMAGE_SIZE=48",
        "config.MODEL.HEAD.num_clusters=16", "config.LOSS.swav_loss.queue.queue_length=4",
        "config.LOSS.swav_loss.queue.start_iter=0", "config.OPTIMIZER.target_batch_size=4",
        "config.OPTIMIZER.batch_size_for_tracking=2",
        "config.MODEL.TEMP_FROZEN_PARAMS_ITER_MAP=[['heads.0.prototypes0.weight', 1]]",
        "config.OPTIMIZER.warmup_epochs=2", "config.OPTIMIZER.max_epochs=10",
        f"config.CHECKPOINT.DIR={tmp_path}",
        "config.MODEL.ACTIVATION_CHECKPOINTING.USE_ACTIVATION_CHECKPOINTING=true",
        "config.MODEL.ACTIVATION_CHECKPOINTING.NUM_ACTIVATION_CHECKPOINTING_SPLITS=8"])
    dht = DHT(start=True)
    with caplog.at_level(logging.INFO, logger="dedloc_amd.training.swav_peer"):
        peer = SwavPeer(cfg, "cpu", dht=dht)
        try:
            assert peer.model.trunk.checkpoint_stages and not peer.use_graph
            losses = [float(peer.train_step()) for _ in range(2)]
            assert all(math.isfinite(x) for x in losses)
            for m in peer.model.trunk.modules():
                if isinstance(m, BNAct):  # two crops per resolution, two resolutions, two steps: once each
                    assert int(m.num_batches_tracked) == 8
        finally:
            peer.shutdown()
            dht.shutdown()
    said = [r for r in caplog.records if "activation checkpointing is on" in r.getMessage()]
    assert len(said) == 1
    assert "concurrent trunk passes" in said[0].getMessage() and "HIP-graph" in said[0].getMessage()
