"""LINEAR_EVAL.PROTOCOL=eval_mlp (training/swav_linear.py): the five-head protocol end to end on a tiny
folder, the NCHW flatten contract of a head's Linear weight, and the features entering every head
(FrozenTrunk.forward_features + the fused pool / BatchNorm path) against fp32 torch."""
import json
import math

import numpy as np
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from dedloc_amd.training import swav_linear as sl
from dedloc_amd.utils.config import load_config
from test_swav_linear import _model, _overrides

TAPS = ("conv1", "res2", "res3", "res4", "res5")
POOLS = {t: (3, 2, 1) for t in TAPS}  # at 64 pixels every stage keeps at least one output


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("eval_mlp_images")
    g = torch.Generator().manual_seed(4)
    for k in range(16):
        d = root / f"class{k % 4}"
        d.mkdir(exist_ok=True)
        np.save(d / f"{k}.npy", torch.randint(0, 256, (40 + 3 * k, 70 - 2 * k, 3), generator=g, dtype=torch.uint8).numpy())
    return root


def test_protocol_defaults_to_the_single_head():
    assert sl.DEFAULTS["PROTOCOL"] == "res5_avgpool" and sl.protocol({}) == "res5_avgpool"
    with pytest.raises(ValueError):
        sl.protocol({"PROTOCOL": "res4_avgpool"})


def test_eval_mlp_end_to_end_cpu(folder, tmp_path):
    model, ckpt = _model(torch.device("cpu")), tmp_path / "heads.torch"
    pools = json.dumps({t: list(POOLS[t]) for t in TAPS})
    over = _overrides(folder) + ["+config.LINEAR_EVAL.PROTOCOL=eval_mlp", f"+config.LINEAR_EVAL.POOLS={pools}",
                                 f"+config.LINEAR_EVAL.SAVE_HEADS={ckpt}"]
    sets = sl.build_linear_sets(load_config("swav_1node_resnet_submit", over))
    recs = sl.linear_evaluate(model, sets, torch.device("cpu"), str(tmp_path / "m.jsonl"))
    assert len(recs) == 2 and [json.loads(l) for l in open(tmp_path / "m.jsonl")] == json.loads(json.dumps(recs))
    out = recs[-1]
    for tap in TAPS:
        for key in ("top1", "top5", "loss"):
            assert math.isfinite(out[f"linear_{key}_{tap}"])
    assert out["linear_top1"] == out["linear_top1_res5"] and out["linear_top5"] == out["linear_top5_res5"]
    assert out["linear_test_images"] == 16 and out["linear_classes"] == 4
    # the heads' widths: C * OH * OW from POOLS over the 64-pixel tap shapes
    sd = torch.load(ckpt, weights_only=True)
    shapes = {"conv1": (64, 32), "res2": (256, 16), "res3": (512, 8), "res4": (1024, 4), "res5": (2048, 2)}
    for tap, (C, hw) in shapes.items():
        k, s, p = POOLS[tap]
        o = (hw + 2 * p - k) // s + 1
        assert sd["heads"][tap]["weight"].shape == (4, C * o * o)
    # round trip: a fresh set of heads loaded from the file saves the same bits
    heads = sl.EvalMLP(4, 64, POOLS)
    heads.load_state_dict(sd)
    again = heads.state_dict()
    for tap in TAPS:
        for k, v in sd["heads"][tap].items():
            assert torch.equal(v, again["heads"][tap][k]), (tap, k)
    # the other protocol's file is refused, both ways
    single = sl.LinearProbe(4)
    with pytest.raises(ValueError, match="protocol"):
        heads.load_state_dict(single.state_dict())
    with pytest.raises(ValueError, match="protocol"):
        single.load_state_dict(sd)
    torch.save(single.state_dict(), tmp_path / "single.torch")
    sets["settings"]["LOAD_HEADS"] = str(tmp_path / "single.torch")
    with pytest.raises(ValueError, match="protocol"):
        sl.linear_evaluate(model, sets, torch.device("cpu"))


def test_head_flattens_in_nchw_order():
    g = torch.Generator().manual_seed(2)
    N, C, hw, classes = 6, 64, 5, 3
    head = sl.EvalMLPHead("res2", (C, hw, hw), (3, 2, 1), classes, "cpu", 7, 0.9, 1e-6)
    with torch.no_grad():
        head.gamma.copy_(torch.empty(C).uniform_(0.5, 1.5, generator=g))
        head.beta.copy_(torch.empty(C).uniform_(-0.5, 0.5, generator=g))
    x = torch.randn(N, C, hw, hw, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    sd = head.state_dict()
    ref = torch.nn.Sequential(torch.nn.BatchNorm2d(C), torch.nn.Flatten(), torch.nn.Linear(head.dim, classes)).double()
    ref[0].load_state_dict({k[3:]: v for k, v in sd.items() if k.startswith("bn.")}, strict=False)
    ref[2].load_state_dict({"weight": sd["weight"], "bias": sd["bias"]})
    pooled = torch.nn.functional.avg_pool2d(x.double(), 3, 2, 1)
    f = head.features(x, True)  # [N, dim] bf16, (oh, ow, c) order
    f_nchw = f.double().reshape(N, head.OH, head.OW, C).permute(0, 3, 1, 2)
    # the BatchNorm stage: pooled values, statistics and the normalisation are fp32; only the stored
    # output is bf16, so each element is within half a bf16 ulp (<= 2^-8 |out|) of BatchNorm2d's, plus
    # an fp32 term.  1e-5 end to end cannot hold through a bf16 f: the Linear stage below takes this f
    bn_want = ref[0].train()(pooled)
    assert ((f_nchw - bn_want).abs() <= 2.0 ** -8 * bn_want.abs() + 1e-5).all()
    # the Linear stage on the same normalised values: the head's weight in its own order over its own
    # rows against torch's Linear with the saved weight over flatten(NCHW)
    want = ref[2](ref[1](f_nchw))
    got = f.double() @ head.probe.weight[:classes].double().T + head.probe.bias[:classes].double()
    err = (got - want).abs().max().item()
    print(f"head vs flatten(NCHW) -> Linear: max abs err {err:.3e}")
    assert err <= 1e-5


def _head_against_torch(device):
    """One training step's BatchNorm gradients and running statistics, then the evaluation-mode features,
    against fp32 BatchNorm2d on the fp32 pooled values.  The channels carry means of 0 to 20 spreads."""
    g = torch.Generator().manual_seed(8)
    N, C, hw = 8, 64, 9
    x = (torch.randn(N, C, hw, hw, generator=g) + torch.linspace(0, 20, C).view(1, C, 1, 1)).bfloat16()
    x = x.to(device).contiguous(memory_format=torch.channels_last)
    labels = (torch.arange(N) % 3).to(device)
    head = sl.EvalMLPHead("res2", (C, hw, hw), (3, 2, 1), 3, device, 7, 0.9, 1e-6)
    bn = torch.nn.BatchNorm2d(C).to(device)
    pooled = torch.nn.functional.avg_pool2d(x.float(), 3, 2, 1)
    w = head._nchw(head.probe.weight.detach()[:3])
    out = bn(pooled)  # gamma 1, beta 0: out is xhat
    out.retain_grad()
    torch.nn.functional.cross_entropy(out.flatten(1) @ w.T + head.probe.bias.detach()[:3], labels).backward()
    head.train_step(x, labels, 0.0)  # lr 0: gradients and running statistics, parameters as they were
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()  # noqa: E731
    # the head rounds f, the Linear weight, the logits and dy to bf16: four relative errors of 2^-9 on
    # every term dy * xhat (dy) of the channel's sum, so 4 * 2^-9 * sum |dy xhat| (sum |dy|) per channel
    mag_g, mag_b = (out.grad * out.detach()).abs().sum(dim=(0, 2, 3)), out.grad.abs().sum(dim=(0, 2, 3))
    errs = dict(dgamma=((head.gamma.grad - bn.weight.grad).abs() / (2.0 ** -7 * mag_g)).max().item(),
                dbeta=((head.beta.grad - bn.bias.grad).abs() / (2.0 ** -7 * mag_b)).max().item(),
                mean=rel(head.running_mean, bn.running_mean), var=rel(head.running_var, bn.running_var))
    with torch.no_grad():
        want = bn.eval()(pooled).permute(0, 2, 3, 1).reshape(N, -1)
    errs["eval"] = ((head.features(x, False).float() - want).abs() / (2.0 ** -8 * want.abs() + 1e-5)).max().item()
    print(f"eval_mlp head vs BatchNorm2d on {device}: {errs}")
    # (errors as fractions of those bounds); the statistics are fp32 sums: 1e-5; the evaluation
    # features: half a bf16 ulp of fp32 BatchNorm2d.eval()
    assert errs["dgamma"] <= 1.0 and errs["dbeta"] <= 1.0 and errs["mean"] <= 1e-5 and errs["var"] <= 1e-5
    assert errs["eval"] <= 1.0


def test_head_step_and_eval_mode_match_batchnorm2d_cpu():
    _head_against_torch(torch.device("cpu"))


@pytest.mark.gpu
def test_head_step_and_eval_mode_match_batchnorm2d_gpu(cuda):
    _head_against_torch(cuda)


@pytest.fixture(scope="module")
def tapped(cuda):
    model = _model(cuda)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(cuda).bfloat16()
    feats = model.frozen_trunk().forward_features(x.contiguous(memory_format=torch.channels_last), TAPS)
    return feats, sl.EvalMLP(4, 64, POOLS, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("tap", TAPS)
def test_head_features_match_fp32_torch_gpu(tapped, tap):
    feats, heads = tapped
    head = heads.heads[TAPS.index(tap)]
    got = head.features(feats[tap], True).float()
    pooled = torch.nn.functional.avg_pool2d(feats[tap].float(), 3, 2, 1)
    want = torch.nn.functional.batch_norm(pooled, None, None, training=True, eps=head.eps)
    want = want.permute(0, 2, 3, 1).reshape(4, -1)
    rel = ((got - want).norm() / want.norm()).item()
    print(f"eval_mlp features {tap}: {tuple(got.shape)}, rel err {rel:.2e}")
    assert got.shape == (4, head.dim) and rel <= 1e-2
