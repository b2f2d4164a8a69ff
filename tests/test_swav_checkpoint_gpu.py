"""Activation checkpointing of the SwAV trunk on the GPU: the bn_apply kernel against bn_fwd, the
replayed segments against the plain trunk (bitwise under DEDLOC_DETERMINISTIC_BN=1, within the
measured run-to-run spread on the default path), what the first pass retains, and that the fused
backward is live in the recompute."""
import collections
import math

import pytest
import torch

from conftest import record_margin
from dedloc_amd.utils.config import load_config

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _img(n, hw, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g).to(torch.bfloat16).contiguous(memory_format=CL).to(dev)


# ------------------------------------------------------------------------------------ 1. bn_apply
@pytest.mark.parametrize("N,C,H,G,relu,res", [
    (8, 64, 28, 1, True, False),     # 6272 rows, 50176 vectors: 196 blocks, one vector per thread
    (16, 256, 7, 1, True, True),
    (4, 2048, 3, 2, False, False),
    (12, 128, 12, 3, True, True),
    (3, 64, 5, 1, True, False),      # 600 vectors: the tail loop in 3 blocks, the last one part-filled
    # past the grid cap (DL_BN_APPLY_MAXB = 768 blocks = 196608 vectors in flight), where the
    # two-vector unrolled loop runs for part of the threads and the tail loop for the rest:
    (8, 256, 32, 1, True, True),     # 262144 vectors in one group
    (8, 256, 32, 2, True, False),    # 131072 per group over 384 blocks each
])
def test_bn_apply_bit_equal_to_bn_fwd(cuda, N, C, H, G, relu, res):
    g = torch.Generator().manual_seed(N * C + H)
    x = (torch.randn(N, C, H, H, generator=g) * 1.5 + 0.3).to(torch.bfloat16).contiguous(memory_format=CL).to(cuda)
    r = torch.randn(N, C, H, H, generator=g).to(torch.bfloat16).contiguous(memory_format=CL).to(cuda) if res else None
    gamma = (torch.rand(C, generator=g) + 0.5).to(cuda)
    beta = torch.randn(C, generator=g).to(cuda)
    rm, rv = torch.randn(C, generator=g).to(cuda), (torch.rand(C, generator=g) + 0.5).to(cuda)
    y, mean, rstd = torch.ops.dedloc.bn_fwd(x, r, gamma, beta, rm, rv, 1e-5, 0.1, relu, G, None, False)
    assert mean.shape == (G, C) and rstd.shape == (G, C)
    kept = [t.clone() for t in (rm, rv, mean, rstd, x)]
    y2 = torch.ops.dedloc.bn_apply(x, r, gamma, beta, mean, rstd, relu, G)
    torch.cuda.synchronize()
    assert y2.dtype == torch.bfloat16 and y2.is_contiguous(memory_format=CL)
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), "bn_apply's y differs from bn_fwd's"
    for t, k in zip((rm, rv, mean, rstd, x), kept):
        assert torch.equal(t, k), "bn_apply wrote one of its inputs / the running statistics"
    if relu:
        assert (y2.float() >= 0).all()


def test_bn_apply_rejects_wrong_statistics_shape(cuda):
    x = torch.randn(4, 64, 4, 4, device=cuda).to(torch.bfloat16).contiguous(memory_format=CL)
    one = torch.ones(64, device=cuda)
    with pytest.raises(RuntimeError, match="mean / rstd"):
        torch.ops.dedloc.bn_apply(x, None, one, one, torch.zeros(1, 64, device=cuda), torch.ones(1, 64, device=cuda),
                                  True, 2)


# ------------------------------------------------------------------------ models under comparison
def _trunk_twins(dev):
    from dedloc_amd.models.resnet_swav import ResNet50Trunk

    torch.manual_seed(0)
    a, b = ResNet50Trunk(checkpoint_stages=True), ResNet50Trunk()
    b.load_state_dict(a.state_dict())
    return a.to(dev).train(), b.to(dev).train()


def _swav(dev, ckpt, state=None):
    """A SwAVModel bound to a flat buffer with the bf16 mirror, as a peer runs it."""
    from dedloc_amd.models.resnet_swav import SwAVModel
    from dedloc_amd.utils.flat import FlatParams

    torch.manual_seed(0)
    m = SwAVModel(num_prototypes=16, single_pass_every_crop=True, checkpoint_stages=ckpt)
    if state is not None:
        m.load_state_dict(state)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m.to(dev).train()
    flat = FlatParams(m.named_parameters(), device=dev, with_bf16=True, autograd=True, channels_last=True)
    m.bind_flat(flat)
    return m, flat, state


def _swav_crops(dev):
    return [_img(2, 64, 1, dev), _img(2, 64, 2, dev), _img(2, 32, 3, dev), _img(2, 32, 4, dev), _img(2, 32, 5, dev)]


def _swav_seed(dev):
    g = torch.Generator().manual_seed(7)
    return (torch.randn(10, 128, generator=g).to(torch.bfloat16).to(dev),
            torch.randn(10, 16, generator=g).to(torch.bfloat16).to(dev))


def _buffers(m):
    return {n: b.clone() for n, b in m.named_buffers()}


def _restore(m, bufs):
    with torch.no_grad():
        for n, b in m.named_buffers():
            b.copy_(bufs[n])


def _swav_run(m, flat, crops, seed):
    flat.grad.zero_()
    e, s = m(crops)
    torch.autograd.backward([e, s], [g.to(t.dtype) for g, t in zip(seed, (e, s))])
    torch.cuda.synchronize()
    return e.clone(), s.clone(), flat.grad.clone(), _buffers(m)


# -------------------------------------------------------------- 2. exact under deterministic BN
def test_trunk_bitwise_under_deterministic_bn(cuda, monkeypatch):
    monkeypatch.setenv("DEDLOC_DETERMINISTIC_BN", "1")
    a, b = _trunk_twins(cuda)
    for it in range(2):
        x = _img(4, 64, 10 + it, cuda)
        ya, yb = a(x), b(x)
        dy = torch.randn(ya.shape, generator=torch.Generator().manual_seed(20 + it)).to(torch.bfloat16).to(cuda)
        ya.backward(dy)
        yb.backward(dy)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), f"iteration {it}: output"
        for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(p, q), f"iteration {it}: buffer {n}"
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(p.grad, q.grad), f"iteration {it}: gradient of {n}"


def test_swav_model_bitwise_under_deterministic_bn(cuda, monkeypatch):
    monkeypatch.setenv("DEDLOC_DETERMINISTIC_BN", "1")
    a, fa, state = _swav(cuda, True)
    b, fb, _ = _swav(cuda, False, state)
    crops, seed = _swav_crops(cuda), _swav_seed(cuda)
    for it in range(2):
        ea, sa, ga, ba = _swav_run(a, fa, crops, seed)
        eb, sb, gb, bb = _swav_run(b, fb, crops, seed)
        assert torch.equal(ea, eb) and torch.equal(sa, sb), f"iteration {it}: embeddings / scores"
        for n in ba:
            assert torch.equal(ba[n], bb[n]), f"iteration {it}: buffer {n}"
        for n in fa.names:
            assert torch.equal(fa.view(ga, n), fb.view(gb, n)), f"iteration {it}: gradient of {n}"


# --------------------------------------------------------------------------- 3. the default path
def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_swav_model_default_path_within_rerun_spread(cuda, monkeypatch):
    """Links and conv-epilogue statistics on: the plain path's statistics are fp32 atomics, so the
    bound is measured — d0 = the largest relative difference of three reruns of the plain model to
    its first run (same state), and the checkpointed model must be within max(4 d0, 2^-8) of that
    first run: 4x because three reruns sample the atomic-order spread thinly, 2^-8 (one bf16 rounding
    step) as the floor when the reruns agree exactly."""
    monkeypatch.delenv("DEDLOC_DETERMINISTIC_BN", raising=False)
    a, fa, state = _swav(cuda, True)
    b, fb, _ = _swav(cuda, False, state)
    crops, seed = _swav_crops(cuda), _swav_seed(cuda)
    start = _buffers(b)

    def stats(bufs):
        return torch.cat([v.float().flatten() for n, v in bufs.items() if "running_" in n])

    def counters(bufs):
        return torch.stack([v for n, v in bufs.items() if n.endswith("num_batches_tracked")])

    runs = []
    for _ in range(4):
        _restore(b, start)
        runs.append(_swav_run(b, fb, crops, seed))
    _restore(a, start)
    ck = _swav_run(a, fa, crops, seed)
    d0_g = max(_rel(r[2], runs[0][2]) for r in runs[1:])
    d0_s = max(_rel(stats(r[3]), stats(runs[0][3])) for r in runs[1:])
    rel_g, rel_s = _rel(ck[2], runs[0][2]), _rel(stats(ck[3]), stats(runs[0][3]))
    bound_g, bound_s = max(4 * d0_g, 2.0 ** -8), max(4 * d0_s, 2.0 ** -8)
    record_margin("swav_checkpoint_default_path", d0_grad=d0_g, rel_grad=rel_g, bound_grad=bound_g,
                  d0_running_stats=d0_s, rel_running_stats=rel_s, bound_running_stats=bound_s)
    print(f"d0_grad={d0_g:.3e} rel_grad={rel_g:.3e} d0_rs={d0_s:.3e} rel_rs={rel_s:.3e}")
    assert torch.equal(counters(ck[3]), counters(runs[0][3]))
    assert math.isfinite(rel_g) and rel_g <= bound_g, (rel_g, d0_g)
    assert math.isfinite(rel_s) and rel_s <= bound_s, (rel_s, d0_s)


# ----------------------------------------------------------------------------- 4. retained memory
def test_first_pass_retains_only_the_boundaries(cuda):
    """retained = memory_allocated after the forward minus before it.  The checkpointed trunk may
    retain what the plain stem (+ max-pool) and the plain layer4 retain on their own, the four
    stage-boundary tensors, and 2 MiB per boundary tensor (the caching allocator's large-block
    rounding) — nothing of layer1-layer3.  The parts are measured here on tensors of the right shape."""
    a, b = _trunk_twins(cuda)
    x = _img(32, 128, 3, cuda)
    for m in (a, b):  # first-call allocations (kernel workspaces) are not activations
        m(x).float().sum().backward()
        m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()

    def retained(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        r = torch.cuda.memory_allocated() - before
        del out
        return r

    def peak(m):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m(x).float().sum().backward()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        m.zero_grad(set_to_none=True)
        return p

    shapes = [(32, 64, 32, 32), (32, 256, 32, 32), (32, 512, 16, 16), (32, 1024, 8, 8)]
    boundary = sum(2 * math.prod(s) for s in shapes)
    r_stem = retained(lambda: b.maxpool(b.bn1(b.conv1(x, b.bn1))))
    x4 = torch.randn(shapes[3], device=cuda).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    r_l4 = retained(lambda: b.layer4(x4))
    r_plain = retained(lambda: b(x))
    r_ckpt = retained(lambda: a(x))
    bound = r_stem + r_l4 + boundary + len(shapes) * (2 << 20)
    p_plain, p_ckpt = peak(b), peak(a)
    record_margin("swav_checkpoint_retained_memory", retained_ckpt=r_ckpt, retained_plain=r_plain, bound=bound,
                  retained_stem=r_stem, retained_layer4=r_l4, boundary_bytes=boundary,
                  peak_fwd_bwd_ckpt=p_ckpt, peak_fwd_bwd_plain=p_plain)
    print(f"retained ckpt={r_ckpt} plain={r_plain} bound={bound}; peak ckpt={p_ckpt} plain={p_plain}")
    assert r_ckpt <= bound, (r_ckpt, bound)
    assert p_ckpt < p_plain, (p_ckpt, p_plain)


# ------------------------------------------------------------------- 5. fused backward is live
def test_fused_backward_runs_in_the_recompute(cuda, monkeypatch):
    """conv2d_dgrad_bn (a BatchNorm's backward preparation in the consuming conv's data gradient)
    runs in the checkpointed backward as often as in the plain one, per stage, minus the links across
    a stage boundary — counted in the plain run (a stage's first block has a shortcut conv, whose
    conv1 takes no such link, so the plain trunk consumes none either)."""
    monkeypatch.delenv("DEDLOC_DETERMINISTIC_BN", raising=False)
    a, b = _trunk_twins(cuda)
    x = _img(4, 64, 5, cuda)
    op = torch.ops.dedloc.conv2d_dgrad_bn
    calls, boundary_x, across = collections.Counter(), [], [0]

    def counted(*args, **kw):
        bx = args[7]  # the linked BatchNorm's input: (channels, height) names its stage
        calls[(bx.shape[1], bx.shape[2])] += 1
        across[0] += any(bx is t for t in boundary_x)
        return op(*args, **kw)

    monkeypatch.setattr(torch.ops.dedloc, "conv2d_dgrad_bn", counted)
    hooks = [s.register_forward_hook(lambda mod, inp, out: boundary_x.append(out._dedloc_bn_link.bn[0]))
             for s in (b.layer1, b.layer2, b.layer3)]
    b(x).float().sum().backward()
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    plain, n_across = dict(calls), across[0]
    assert len(boundary_x) == 3 and sum(plain.values()) > 0
    calls.clear()
    boundary_x.clear()
    a(x).float().sum().backward()
    torch.cuda.synchronize()
    ckpt = dict(calls)
    assert sum(ckpt.values()) == sum(plain.values()) - n_across
    if n_across == 0:
        assert ckpt == plain  # stage by stage
    layer4 = {(512, 2), (2048, 2)}
    assert sum(v for k, v in ckpt.items() if k not in layer4) > 0


# --------------------------------------------------------------------------------------- 6. peer
def test_peer_gpu_steps_with_checkpointing(cuda, tmp_path):
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer

    cfg = load_config("swav_1node_resnet_submit", [
        "config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=8", "config.DATA.TRAIN.SYNTHETIC_POOL_SIZE=16",
        "config.LOSS.swav_loss.queue.start_iter=0", "config.LOSS.swav_loss.queue.queue_length=64",
        "config.OPTIMIZER.target_batch_size=16", "config.OPTIMIZER.batch_size_for_tracking=8",
        f"config.CHECKPOINT.DIR={tmp_path}", "config.MODEL.CUDA_GRAPH=true", "config.MODEL.CONCURRENT_PASSES=true",
        "config.MODEL.ACTIVATION_CHECKPOINTING.USE_ACTIVATION_CHECKPOINTING=true"])
    dht = DHT(start=True)
    peer = SwavPeer(cfg, cuda, dht=dht)
    try:
        assert peer.use_graph is False and peer.model.concurrent_passes and peer.model.trunk.checkpoint_stages
        losses = [float(peer.train_step()) for _ in range(3)]
        assert all(math.isfinite(v) for v in losses), losses
        assert peer._graphed is None
        assert getattr(peer.model, "_conc", None) is None  # _trunk_concurrent never ran
    finally:
        peer.shutdown()
        dht.shutdown()
