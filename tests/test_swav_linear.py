"""Linear evaluation of a SwAV model (training/swav_linear.py, cli/linear_swav.py): the schedules, the
random-resized-crop parameter table, the head-training loop against a torch.nn.Linear + SGD
reimplementation, and the whole evaluation end to end on a tiny folder."""
import json
import math

import numpy as np
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from dedloc_amd.data.multicrop import MultiCropAugment
from dedloc_amd.training.swav_linear import LinearProbe, build_linear_sets, learning_rate, linear_evaluate, train_linear
from dedloc_amd.utils.config import load_config


def test_schedules_equal_their_closed_forms():
    epochs, spe, peak = 3, 4, 0.3 * 8 / 256
    for step in range(epochs * spe):
        want = peak * (1 + math.cos(math.pi * step / (epochs * spe))) / 2
        assert learning_rate(step, spe, epochs, peak) == pytest.approx(want, rel=1e-12, abs=0)
    assert learning_rate(0, spe, epochs, peak) == peak
    values, milestones = [1.0, 0.1, 0.01], [1, 2]
    for step in range(epochs * spe):
        want = peak * values[sum(step // spe >= m for m in milestones)]
        assert learning_rate(step, spe, epochs, peak, "multistep", values, milestones) == want
    with pytest.raises(ValueError):
        learning_rate(0, spe, epochs, peak, "multistep", [1.0], [1, 2])
    with pytest.raises(ValueError):
        learning_rate(0, spe, epochs, peak, "linear")


def test_crop_flip_table_obeys_its_bounds():
    n = 10000
    g = torch.Generator().manual_seed(0)
    H = torch.randint(33, 400, (n,), generator=g)
    W = torch.randint(33, 400, (n,), generator=g)
    src = torch.arange(n) % 7
    p = MultiCropAugment.crop_flip_params(src, H, W, torch.Generator().manual_seed(1)).double()
    assert p.shape == (n, 20) and torch.equal(p[:, 0], src.double())
    left, top, w, h = p[:, 1], p[:, 2], p[:, 3].abs(), p[:, 4]
    Hd, Wd = H.double(), W.double()
    assert (left >= 0).all() and (top >= 0).all() and (w >= 1).all() and (h >= 1).all()
    assert (left + w <= Wd).all() and (top + h <= Hd).all()  # inside the image
    assert torch.equal(p[:, 1:5], p[:, 1:5].round())  # whole pixels
    # torchvision's fallback (no attempt of ten fits): the centred box of the clamped image ratio
    ratio = Wd / Hd
    fw = torch.where(ratio > 4 / 3, torch.round(Hd * (4 / 3)), Wd)
    fh = torch.where(ratio < 3 / 4, torch.round(Wd / (3 / 4)), Hd)
    fallback = (w == fw) & (h == fh) & (left == torch.floor((Wd - w) / 2)) & (top == torch.floor((Hd - h) / 2))
    ok = ~fallback
    assert ok.float().mean() > 0.9
    # w = round(sqrt(area * r)), h = round(sqrt(area / r)): each within half a pixel of its real value
    frac = (w * h) / (Hd * Wd)
    lo = ((w - 0.5) * (h - 0.5)) / (Hd * Wd)
    hi = ((w + 0.5) * (h + 0.5)) / (Hd * Wd)
    assert (hi[ok] >= 0.08).all() and (lo[ok] <= 1.0).all() and (frac[ok] <= 1.0).all()
    assert (((w + 0.5) / (h - 0.5))[ok] >= 3 / 4).all() and (((w - 0.5) / (h + 0.5))[ok] <= 4 / 3).all()
    flips = (p[:, 3] < 0).double().mean().item()
    assert abs(flips - 0.5) < 4 * 0.5 / math.sqrt(n)  # four standard deviations of a fair coin
    # colour and blur columns at identity, as center_params
    ident = MultiCropAugment.center_params(src, H, W, 224, 256).double()
    assert torch.equal(p[:, 5:], ident[:, 5:])


class _FeatureStream:
    """Fixed features in place of images (the extractor is the identity)."""

    def __init__(self, f, y, batch, shuffle_seed=None):
        self.f, self.y, self.batch, self.seed = f, y, batch, shuffle_seed

    def __len__(self):
        return self.f.shape[0]

    def steps_per_epoch(self):
        return -(-len(self) // self.batch)

    def order(self, e):
        if self.seed is None:
            return torch.arange(len(self))
        return torch.randperm(len(self), generator=torch.Generator().manual_seed(self.seed + e))

    def epoch(self, e):
        o = self.order(e)
        for s in range(0, len(self), self.batch):
            yield self.f[o[s:s + self.batch]], self.y[o[s:s + self.batch]]

    def __iter__(self):
        return self.epoch(0)


def test_head_training_matches_a_torch_reimplementation():
    g = torch.Generator().manual_seed(3)
    y = torch.arange(16) % 2
    direction = torch.randn(2048, generator=g)
    f = (0.1 * torch.randn(16, 2048, generator=g) + (2.0 * y.float() - 1)[:, None] * direction * 0.05).bfloat16()
    train, test = _FeatureStream(f, y, 8, shuffle_seed=5), _FeatureStream(f, y, 8)
    settings = dict(NUM_EPOCHS=10, BATCH_SIZE=8, TEST_EVERY_NUM_EPOCH=1)  # 10 epochs x 2 batches = 20 steps
    probe = LinearProbe(2, device="cpu", seed=11)
    ref = torch.nn.Linear(2048, 2)
    with torch.no_grad():
        ref.weight.copy_(probe.weight[:2])
        ref.bias.copy_(probe.bias[:2])
    w0 = probe.weight[:2].detach().clone()
    recs = train_linear(lambda t: t, train, test, 2, settings, "cpu", probe=probe)
    opt = torch.optim.SGD(ref.parameters(), lr=0.0, momentum=0.9, weight_decay=1e-6, nesterov=False)
    peak, step = 0.3 * 8 / 256, 0
    for e in range(10):
        for xb, yb in train.epoch(e):
            for gp in opt.param_groups:
                gp["lr"] = learning_rate(step, 2, 10, peak)
            opt.zero_grad()
            torch.nn.functional.cross_entropy(ref(xb.float()), yb).backward()
            opt.step()
            step += 1
    assert step == 20
    dw = (probe.weight[:2].detach() - ref.weight.detach()).abs().max().item()
    db = (probe.bias[:2].detach() - ref.bias.detach()).abs().max().item()
    moved = (probe.weight[:2].detach() - w0).abs().max().item()
    print(f"linear head vs torch fp32 after 20 steps: max |dW| {dw:.3e}, max |db| {db:.3e}, weights moved {moved:.3e}")
    # measured on the CPU: max |dW| 1.082e-05, max |db| 2.240e-05 (the head reads its weights and writes
    # its logits and their gradients in bf16; the fp32 reimplementation does not) -> asserted at 2x
    assert dw <= 2 * 1.082e-05 and db <= 2 * 2.240e-05, (dw, db)
    assert moved > 100 * dw  # the agreement is of trained weights, not of the shared init
    assert (probe.weight[2:] == 0).all() and (probe.bias[2:] == 0).all()  # the padded rows never move
    assert len(recs) == 10 and recs[-1]["linear_epoch"] == 10
    assert recs[-1]["linear_train_loss"] < recs[0]["linear_train_loss"] and recs[-1]["linear_loss"] < recs[0]["linear_loss"]
    assert recs[-1]["linear_top1"] == 1.0 and recs[-1]["linear_top5"] == 1.0
    assert recs[-1]["linear_test_images"] == 16 and recs[-1]["linear_classes"] == 2


@pytest.mark.parametrize("classes", [2, 5, 8, 11])
def test_any_class_count_trains(classes):
    g = torch.Generator().manual_seed(classes)
    y = torch.arange(24) % classes
    f = torch.randn(24, 2048, generator=g).bfloat16()
    s = _FeatureStream(f, y, 8)
    recs = train_linear(lambda t: t, s, s, classes, dict(NUM_EPOCHS=2, BATCH_SIZE=8), "cpu")
    assert recs[-1]["linear_classes"] == classes and math.isfinite(recs[-1]["linear_loss"])
    assert 0.0 <= recs[-1]["linear_top1"] <= recs[-1]["linear_top5"] <= 1.0
    with pytest.raises(ValueError):
        LinearProbe(1)


# ------------------------------------------------------------------ end to end
KEYS = {"linear_top1", "linear_top5", "linear_loss", "linear_epoch", "linear_train_images", "linear_test_images",
        "linear_classes"}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("linear_images")
    g = torch.Generator().manual_seed(9)
    for k, (h, w) in enumerate([(40, 56), (64, 64), (33, 91), (75, 50), (48, 48), (101, 37), (57, 57), (80, 120)]):
        d = root / f"class{k % 2}"
        d.mkdir(exist_ok=True)
        np.save(d / f"{k}.npy", torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())
    return root


def _overrides(folder):
    return ["config.DATA.TRAIN.DATA_SOURCES=[disk_folder]", f'+config.DATA.TRAIN.DATA_PATHS=["{folder}"]',
            "+config.DATA.TEST.DATA_SOURCES=[disk_folder]", f'+config.DATA.TEST.DATA_PATHS=["{folder}"]',
            "config.DATA.TRAIN.NUM_DATALOADER_WORKERS=2", "config.MODEL.HEAD.num_clusters=16",
            "+config.LINEAR_EVAL.NUM_EPOCHS=2", "+config.LINEAR_EVAL.BATCH_SIZE=4", "+config.LINEAR_EVAL.CROP_SIZE=64",
            "+config.LINEAR_EVAL.CENTER_CROP=64", "+config.LINEAR_EVAL.RESIZE=72"]


def _model(device):
    from dedloc_amd.models.resnet_swav import SwAVModel

    torch.manual_seed(0)
    model = SwAVModel(num_prototypes=16).to(device)
    model.train()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.8, 1.2)
                m.num_batches_tracked.fill_(3)
    return model


def _end_to_end(device, folder, tmp_path, runs):
    model = _model(device)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cfg = load_config("swav_1node_resnet_submit", _overrides(folder))
    outs = []
    for r in range(runs):
        mf = tmp_path / f"metrics_{device.type}_{r}.jsonl"
        recs = linear_evaluate(model, build_linear_sets(cfg), device, str(mf))
        lines = [json.loads(l) for l in open(mf)]
        assert lines == [json.loads(json.dumps(x)) for x in recs] and len(recs) == 2
        out = recs[-1]
        assert KEYS <= set(out) and out["eval"] is True
        assert 0.0 <= out["linear_top1"] <= out["linear_top5"] <= 1.0 and math.isfinite(out["linear_loss"])
        assert out["linear_test_images"] == 8 and out["linear_train_images"] == 8
        assert out["linear_classes"] == 2 and out["linear_epoch"] == 2
        outs.append(json.dumps(recs))
    assert model.training
    after = model.state_dict()
    assert before.keys() == after.keys()
    for k in before:  # trunk and head projection: parameters, running statistics, counters
        assert torch.equal(before[k], after[k]), k
    return outs


def test_linear_evaluation_end_to_end_cpu(folder, tmp_path):
    a, b = _end_to_end(torch.device("cpu"), folder, tmp_path, 2)
    assert a == b  # two runs, the same JSON


@pytest.mark.gpu
def test_linear_evaluation_end_to_end_gpu(cuda, folder, tmp_path):
    _end_to_end(cuda, folder, tmp_path, 1)


def _cli(device, folder, tmp_path, capsys):
    from dedloc_amd.cli import linear_swav

    model = _model(device)
    ckpt = tmp_path / "model.torch"
    torch.save({"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "iteration": 7,
                "collab_step": 2}, ckpt)
    mf = tmp_path / "cli_metrics.jsonl"
    out = linear_swav.main(["config=pretrain/swav/swav_1node_resnet_submit", f"+config.CHECKPOINT.PATH={ckpt}",
                            f"config.METRICS_FILE={mf}"] + _overrides(folder) + ["--device", str(device)])
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(printed) == 1 and json.loads(printed[0]) == out
    assert KEYS <= set(out) and out["iteration"] == 7 and out["step"] == 2 and out["linear_test_images"] == 8
    assert len(open(mf).read().splitlines()) == 2


def test_linear_swav_cli_prints_one_json_line_cpu(folder, tmp_path, capsys):
    _cli(torch.device("cpu"), folder, tmp_path, capsys)


@pytest.mark.gpu
def test_linear_swav_cli_prints_one_json_line_gpu(cuda, folder, tmp_path, capsys):
    _cli(cuda, folder, tmp_path, capsys)
