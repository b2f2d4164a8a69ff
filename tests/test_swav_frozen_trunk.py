"""SwAVModel.frozen_trunk(): the inference snapshot of the trunk (BatchNorm folded into the convs'
epilogues, conv2d_bn_act) against the model's own eval() forward and an fp32 reference, and its
opt-in use by the kNN evaluation."""
import numpy as np
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from conftest import record_margin
from dedloc_amd.models.resnet_swav import FrozenTrunk, SwAVModel
from dedloc_amd.training.swav_eager import eager_twin

CL = torch.channels_last


def _model(device, seed=0):
    torch.manual_seed(seed)
    model = SwAVModel(num_prototypes=16).to(device)
    model.train()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # running statistics and affine parameters that are not the initial ones
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                n = m.num_features
                m.running_mean.copy_(torch.empty(n).uniform_(-0.1, 0.1, generator=g))
                m.running_var.copy_(torch.empty(n).uniform_(0.8, 1.2, generator=g))
                m.weight.copy_(torch.empty(n).uniform_(0.8, 1.2, generator=g))
                m.bias.copy_(torch.empty(n).uniform_(-0.1, 0.1, generator=g))
                m.num_batches_tracked.fill_(3)
    return model


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _check_against_fp32(device):
    """Both forwards against the fp32 eval-mode reference of the same weights: the frozen path's
    relative error is held to 1.3x the existing path's (the standing ours-vs-stock margin of
    tests/test_swav_parity_gpu.py)."""
    model = _model(device)
    ref = eager_twin(model, device=device).eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    out = []
    for n, hw in ((4, 64), (3, 96)):  # 96: the layer-4 spatial size is 3, odd
        x = torch.randn(n, 3, hw, hw, generator=torch.Generator().manual_seed(hw)).to(device)
        x = x.bfloat16().contiguous(memory_format=CL)
        with torch.no_grad():
            want = ref.trunk(x.float())
        frozen = model.frozen_trunk()
        assert isinstance(frozen, FrozenTrunk)
        f = frozen(x)
        assert model.training  # untouched by the snapshot and its call
        model.eval()
        with torch.no_grad(), torch.autocast(device_type=x.device.type, dtype=torch.bfloat16, enabled=x.is_cuda):
            e = model.features(x)
        model.train()
        assert f.shape == (n, 2048) and f.dtype == torch.bfloat16 and f.grad_fn is None and not f.requires_grad
        ef, ee = _rel(f, want), _rel(e, want)
        print(f"frozen trunk {device} {n}x{hw}: rel err frozen {ef:.5f}, eval() path {ee:.5f}, ratio {ef / ee:.3f}")
        out.append((n, hw, ef, ee))
        assert ef <= 1.3 * ee, (ef, ee)
        two = model.frozen_trunk(fused=False)(x)  # the two-kernel form computes the same bits
        assert torch.equal(two.view(torch.int16), f.view(torch.int16))
    after = model.state_dict()
    assert before.keys() == after.keys() and model.training
    for k in before:
        assert torch.equal(before[k], after[k]), k
    return out


def test_frozen_trunk_matches_fp32_cpu():
    _check_against_fp32(torch.device("cpu"))


@pytest.mark.gpu
def test_frozen_trunk_matches_fp32_gpu(cuda):
    for n, hw, ef, ee in _check_against_fp32(cuda):
        record_margin("frozen_trunk_vs_fp32", images=n, size=hw, rel_err_frozen=ef, rel_err_eval_path=ee,
                      bound_ratio=1.3)


def test_frozen_trunk_is_a_snapshot():
    model = _model("cpu")
    frozen = model.frozen_trunk()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).bfloat16().contiguous(memory_format=CL)
    a = frozen(x)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.5)
        model.trunk.bn1.running_mean.add_(1.0)
    assert torch.equal(frozen(x), a)  # holds nothing of the model
    assert not torch.equal(model.frozen_trunk()(x), a)
    with pytest.raises(ValueError):
        frozen(x.float())
    with pytest.raises(ValueError):
        model.frozen_trunk(fused=("5x5",))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("frozen_images")
    g = torch.Generator().manual_seed(9)
    for k, (h, w) in enumerate([(40, 56), (64, 64), (33, 91), (75, 50), (48, 48), (101, 37), (57, 57), (80, 120)]):
        d = root / f"class{k % 2}"
        d.mkdir(exist_ok=True)
        np.save(d / f"{k}.npy", torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())
    return root


def _features_both_ways(device, folder):
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderEvalStream
    from dedloc_amd.training.swav_eval import build_knn_sets, extract_features, knn_evaluate_sets
    from dedloc_amd.utils.config import load_config

    model = _model(device)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ds = ImageFolderDataset([str(folder)])
    stream = ImageFolderEvalStream(ds, 3, device, size=64, resize=72, num_workers=2)
    for feature, D in (("trunk", 2048), ("head", 128)):
        f0, y0 = extract_features(model, stream, feature)
        f1, y1 = extract_features(model, stream, feature, frozen=True)
        assert f0.shape == f1.shape == (8, D) and f1.dtype == torch.bfloat16 and f1.grad_fn is None
        assert y0.tolist() == y1.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
        assert (f1.float().norm(dim=1) - 1).abs().max() < 2 ** -7
        assert (f0.float().norm(dim=1) - 1).abs().max() < 2 ** -7
    stream.close()
    outs = []
    for frozen in (False, True):
        cfg = load_config("swav_1node_resnet_submit", [
            "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]", f'+config.DATA.TRAIN.DATA_PATHS=["{folder}"]',
            "+config.DATA.TEST.DATA_SOURCES=[disk_folder]", f'+config.DATA.TEST.DATA_PATHS=["{folder}"]',
            "+config.NEAREST_NEIGHBOR.CENTER_CROP=64", "+config.NEAREST_NEIGHBOR.RESIZE=72",
            "config.DATA.TRAIN.NUM_DATALOADER_WORKERS=2"]
            + (["+config.NEAREST_NEIGHBOR.FROZEN_TRUNK=True"] if frozen else []))
        sets = build_knn_sets(cfg)
        assert sets["frozen"] is frozen
        outs.append(knn_evaluate_sets(model, sets, device))
    assert outs[0].keys() == outs[1].keys()
    assert outs[1]["knn_samples"] == 8 and outs[1]["knn_bank"] == 8 and 0.0 <= outs[1]["knn_top1"] <= 1.0
    assert model.training
    after = model.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_extract_features_frozen_cpu(folder):
    _features_both_ways(torch.device("cpu"), folder)


@pytest.mark.gpu
def test_extract_features_frozen_gpu(cuda, folder):
    _features_both_ways(cuda, folder)
