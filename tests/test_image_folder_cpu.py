"""The disk_folder SwAV source on the CPU: RandomResizedCrop draws in pixels, the ragged multi-crop
reference op, the image-folder dataset and stream, and the peer / launcher wiring."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dedloc_amd.ops  # noqa: F401
from dedloc_amd.data.multicrop import MultiCropAugment, augment_reference_ragged
from dedloc_amd.utils.config import load_config, parse_cli


def _noise_images(sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _pack(images):
    sizes = [im.numel() for im in images]
    off = np.cumsum([0] + sizes[:-1])
    meta = torch.tensor([[int(o), im.shape[0], im.shape[1]] for o, im in zip(off, images)], dtype=torch.int64)
    return torch.cat([im.reshape(-1) for im in images]), meta


# ------------------------------------------------------------------ host draws
@pytest.mark.parametrize("H,W", [(375, 500), (64, 64)])
@pytest.mark.parametrize("scale", [(0.14, 1.0), (0.05, 0.14)])
def test_ragged_draw_statistics(H, W, scale):
    aug = MultiCropAugment()
    n = 20000
    gen = torch.Generator().manual_seed(0)
    p = aug.sample_params_ragged(torch.zeros(n, dtype=torch.long), torch.full((n,), H), torch.full((n,), W), scale, gen)
    assert p.shape == (n, 20) and torch.equal(p[:, :5], p[:, :5].round())  # integers stored as floats
    j, i, w, h = p[:, 1], p[:, 2], p[:, 3].abs(), p[:, 4]
    assert (w >= 1).all() and (h >= 1).all() and (j >= 0).all() and (i >= 0).all()
    assert (j + w <= W).all() and (i + h <= H).all()
    # the centred fallback box: the whole image here (both ratios lie inside [3/4, 4/3])
    fallback = (w == W) & (h == H) & (j == 0) & (i == 0)
    assert fallback.float().mean() <= 0.01
    # w = round(sqrt(a r)), h = round(sqrt(a / r)): each within 0.5 of its real value, so
    # |w h - a| <= 0.5 (w + h) + 0.25
    area, tol = (w * h)[~fallback], (0.5 * (w + h) + 0.25)[~fallback]
    assert (area >= scale[0] * H * W - tol).all() and (area <= scale[1] * H * W + tol).all()
    ratio = (w / h)[~fallback]
    assert ratio.min() > 0.6 and ratio.max() < 1.6
    assert abs((p[:, 3] < 0).float().mean() - 0.5) < 0.02
    assert abs(p[:, 8].mean() - 0.8) < 0.02 and abs(p[:, 9].mean() - 0.2) < 0.02
    assert abs((p[:, 19] > 0).float().mean() - 0.5) < 0.02
    assert torch.allclose(p[0, 10:19].view(3, 3).sum(1), torch.ones(3), atol=1e-4)


def test_ragged_draw_fallback_is_the_centred_clamped_box():
    """20 x 400 with scale (0.14, 1): no attempt fits (h <= 20 needs an aspect ratio above 4/3 at
    every area), so every draw is the centred box with ratio 4/3: w = round(20 * 4/3) = 27, h = 20."""
    aug = MultiCropAugment()
    n = 2000
    p = aug.sample_params_ragged(torch.zeros(n, dtype=torch.long), torch.full((n,), 20), torch.full((n,), 400),
                                 (0.14, 1.0), torch.Generator().manual_seed(1))
    assert (p[:, 3].abs() == 27).all() and (p[:, 4] == 20).all()
    assert (p[:, 1] == (400 - 27) // 2).all() and (p[:, 2] == 0).all()


# ------------------------------------------------------------------ the CPU op
def test_ragged_reference_op_matches_an_independent_composition():
    images = _noise_images([(7, 5), (33, 64), (120, 90)])
    data, meta = _pack(images)
    aug = MultiCropAugment()
    gen = torch.Generator().manual_seed(2)
    src = torch.tensor([0, 1, 2, 2, 1, 0, 2, 1])
    H, W = meta[src, 1], meta[src, 2]
    size = 24
    params = aug.sample_params_ragged(src, H, W, (0.14, 1.0), gen)
    params[:, 5:8] = 1.0
    params[:, 8:10] = 0.0
    params[:, 19] = 0.0
    out = torch.ops.dedloc.multicrop_ragged(data, meta, params, size, aug.rad, list(aug.mean), list(aug.std))
    assert out.dtype == torch.bfloat16 and out.shape == (8, 3, size, size)
    assert out.is_contiguous(memory_format=torch.channels_last)
    # before the bf16 cast: the shared tail with the identity colour / blur is Normalize alone
    from dedloc_amd.data.multicrop import crop_resize_ragged

    got = crop_resize_ragged(data, meta, params, size)
    mean, std = torch.tensor(aug.mean).view(1, 3, 1, 1), torch.tensor(aug.std).view(1, 3, 1, 1)
    for k in range(8):
        im = images[int(src[k])]
        j, i, w, h = (int(v) for v in params[k, 1:5])
        crop = im[i:i + h, j:j + abs(w)].permute(2, 0, 1)[None].float() / 255
        ref = F.interpolate(crop, size=(size, size), mode="bilinear", antialias=True, align_corners=False)
        if w < 0:
            ref = torch.flip(ref, dims=[3])
        assert (got[k] - ref[0]).abs().max() < 1e-5
        full = (ref - mean) / std
        assert (out[k].float() - full[0].bfloat16().float()).abs().max() < 1e-5 + 2 ** -7 * full.abs().max()
    assert torch.equal(out, augment_reference_ragged(data, meta, params, size, aug.rad, aug.mean, aug.std))


def test_ragged_reference_op_clamps_bad_rows():
    data, meta = _pack(_noise_images([(9, 11), (6, 4)]))
    aug = MultiCropAugment()
    params = aug.sample_params_ragged(torch.tensor([0, 1, 1]), meta[[0, 1, 1], 1], meta[[0, 1, 1], 2], (0.14, 1.0),
                                      torch.Generator().manual_seed(0))
    params[0, 0] = 7        # no such image row
    params[1, 1:5] = torch.tensor([100.0, -3.0, 50.0, 0.0])  # box outside the image
    bad_meta = meta.clone()
    bad_meta[1] = torch.tensor([10 ** 9, 0, 4])  # offset past the buffer, H = 0
    out = torch.ops.dedloc.multicrop_ragged(data, bad_meta, params, 8, aug.rad, list(aug.mean), list(aug.std))
    assert torch.isfinite(out.float()).all()


# ------------------------------------------------------------------ dataset and stream
def _write_npy_folder(root, sizes, seed=0):
    images = _noise_images(sizes, seed)
    for k, im in enumerate(images):
        d = root / f"class{k % 3}"
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / f"img{k:02d}.npy", im.numpy())
    return images


def test_dataset_serves_npy_byte_exact_sorted_recursive(tmp_path):
    from dedloc_amd.data.image_folder import ImageFolderDataset

    images = _write_npy_folder(tmp_path, [(9, 7), (5, 12), (30, 20), (8, 8)])
    (tmp_path / "notes.txt").write_text("not an image")
    ds = ImageFolderDataset([str(tmp_path)])
    assert len(ds) == 4 and ds.files == sorted(ds.files)
    by_name = {f"img{k:02d}.npy": im for k, im in enumerate(images)}
    for k, path in enumerate(ds.files):
        got = ds.load(k)
        assert got.dtype == np.uint8 and np.array_equal(got, by_name[path.rsplit("/", 1)[1]].numpy())
    assert ds.num_replaced == 0
    with pytest.raises(FileNotFoundError):
        ImageFolderDataset([str(tmp_path / "class0" / "missing")])


def test_dataset_decodes_png_byte_exact(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dedloc_amd.data.image_folder import ImageFolderDataset

    images = _noise_images([(10, 14), (21, 6)])
    (tmp_path / "a" / "b").mkdir(parents=True)
    Image.fromarray(images[0].numpy()).save(tmp_path / "a" / "b" / "deep.png")
    Image.fromarray(images[1].numpy()).save(tmp_path / "top.PNG")
    np.save(tmp_path / "a" / "pre.npy", images[0].numpy())
    ds = ImageFolderDataset(str(tmp_path))
    assert [p[len(str(tmp_path)) + 1:] for p in ds.files] == ["a/b/deep.png", "a/pre.npy", "top.PNG"]
    assert np.array_equal(ds.load(0), images[0].numpy()) and np.array_equal(ds.load(1), images[0].numpy())
    assert np.array_equal(ds.load(2), images[1].numpy())


def test_dataset_replaces_a_truncated_file_by_grey_and_counts_it(tmp_path, caplog):
    Image = pytest.importorskip("PIL.Image")
    from dedloc_amd.data.image_folder import ImageFolderDataset

    im = _noise_images([(40, 40)])[0]
    Image.fromarray(im.numpy()).save(tmp_path / "ok.png")
    blob = (tmp_path / "ok.png").read_bytes()
    (tmp_path / "cut.png").write_bytes(blob[: len(blob) // 2])
    ds = ImageFolderDataset([str(tmp_path)])
    with caplog.at_level("WARNING"):
        grey = ds.load(0)
        ds.load(0)
    assert grey.shape == (224, 224, 3) and (grey == 128).all()
    assert ds.num_replaced == 2 and np.array_equal(ds.load(1), im.numpy())
    assert sum("cut.png" in r.getMessage() for r in caplog.records) == 1  # logged once per path


def test_dataset_honours_max_image_side(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dedloc_amd.data.image_folder import ImageFolderDataset

    big = _noise_images([(90, 300)])[0]
    Image.fromarray(big.numpy()).save(tmp_path / "big.jpg", quality=90)
    Image.fromarray(big.numpy()).save(tmp_path / "big.png")
    np.save(tmp_path / "big.npy", big.numpy())
    ds = ImageFolderDataset([str(tmp_path)], max_image_side=64)
    for k in range(3):
        assert ds.load(k).shape == (19, 64, 3)
    assert ImageFolderDataset([str(tmp_path)], max_image_side=512).load(1).shape == (90, 300, 3)


def _stream(root, batch, seed, **kw):
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderMultiCropStream

    aug = MultiCropAugment(size_crops=(32, 16), num_crops=(2, 3))
    return ImageFolderMultiCropStream(batch, "cpu", ImageFolderDataset([str(root)]), seed=seed, augment=aug,
                                      out_dtype=torch.float32, num_workers=3, **kw)


def test_stream_shapes_and_same_seed_gives_equal_batches(tmp_path):
    _write_npy_folder(tmp_path, [(20, 31), (64, 48), (7, 5), (33, 33), (50, 80)])
    a, b, c = _stream(tmp_path, 3, 4), _stream(tmp_path, 3, 4, prefetch_batches=0), _stream(tmp_path, 3, 5)
    assert a.batch_size == 3 and a.augment.size_crops == [32, 16]
    first = None
    for _ in range(3):  # runs across an epoch boundary (5 images, batch 3)
        x, y = a.next_batch(), b.next_batch()
        first = first or x
        assert [tuple(t.shape) for t in x] == [(3, 3, 32, 32)] * 2 + [(3, 3, 16, 16)] * 3
        assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in x)
        assert x[0].is_contiguous(memory_format=torch.channels_last)
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    assert not all(torch.equal(s, t) for s, t in zip(first, c.next_batch()))
    for s in (a, b, c):
        s.close()


def test_stream_serves_every_image_once_per_epoch(tmp_path):
    """10 images at batch 4: constant images whose value is their index, so the crops' mean tells
    which image each sample was cut from."""
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderMultiCropStream

    for k in range(10):
        np.save(tmp_path / f"{k}.npy", np.full((12 + k, 17, 3), 20 * k, dtype=np.uint8))
    aug = MultiCropAugment(size_crops=(8,), num_crops=(1,), crop_scales=((0.5, 1.0),), color_p=0.0, gray_p=0.0,
                           blur_p=0.0, mean=(0, 0, 0), std=(1, 1, 1))
    s = ImageFolderMultiCropStream(4, "cpu", ImageFolderDataset([str(tmp_path)]), seed=3, augment=aug,
                                   out_dtype=torch.float32, num_workers=2)
    seen = []
    for _ in range(5):
        (crop,) = s.next_batch()
        seen.extend(int(round(float(v) * 255 / 20)) for v in crop.mean(dim=(1, 2, 3)))
    s.close()
    assert sorted(seen[:10]) == list(range(10)) and sorted(seen[10:]) == list(range(10))
    assert seen[:10] != seen[10:]  # reshuffled (one chance in 10! of a false alarm, fixed by the seed)


# ------------------------------------------------------------------ peer and launcher
def _tiny_cfg(extra=()):  # tests/test_swav.py::_tiny_cfg
    return load_config("swav_1node_resnet_submit", [
        "config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=2", "config.DATA.TRAIN.MULTICROP.size_crops=[32,16]",
        "config.DATA.TRAIN.MULTICROP.num_crops=[2,2]",
        "config.DATA.TRAIN.SYNTHETIC_POOL_SIZE=4", "config.DATA.TRAIN.SYNTHETIC_IMAGE_SIZE=48",
        "config.MODEL.HEAD.num_clusters=16", "config.LOSS.swav_loss.queue.queue_length=4",
        "config.LOSS.swav_loss.queue.start_iter=0", "config.OPTIMIZER.target_batch_size=4",
        "config.OPTIMIZER.batch_size_for_tracking=2",
        "config.MODEL.TEMP_FROZEN_PARAMS_ITER_MAP=[['heads.0.prototypes0.weight', 1]]",
        "config.OPTIMIZER.warmup_epochs=2", "config.OPTIMIZER.max_epochs=10", *extra])


def test_reference_override_spelling_parses():
    name, ov, rest = parse_cli(["config=pretrain/swav/swav_1node_resnet_submit",
                                "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]",
                                '+config.DATA.TRAIN.DATA_PATHS=["/data/train"]',
                                "config.DATA.TRAIN.DATASET_NAMES=[imagenet1k_folder]", "--max_iterations", "3"])
    assert rest == ["--max_iterations", "3"]
    cfg = load_config(name, ov)
    assert cfg.DATA.TRAIN.DATA_SOURCES == ["disk_folder"] and cfg.DATA.TRAIN.DATA_PATHS == ["/data/train"]
    default = load_config(name, [])
    assert default.DATA.TRAIN.DATA_SOURCES == ["synthetic"]  # the shipped default stays synthetic
    assert default.DATA.TRAIN.NUM_DATALOADER_WORKERS == 8 and default.DATA.TRAIN.MAX_IMAGE_SIDE == 512


def test_swav_peer_cpu_runs_on_a_disk_folder(tmp_path):
    from dedloc_amd.data.image_folder import ImageFolderMultiCropStream
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer

    data = tmp_path / "train"
    _write_npy_folder(data, [(40, 52), (64, 64), (33, 90), (75, 50), (48, 48), (100, 37)])
    cfg = _tiny_cfg([f"config.CHECKPOINT.DIR={tmp_path}", "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]",
                     f'+config.DATA.TRAIN.DATA_PATHS=["{data}"]'])
    dht = DHT(start=True)
    peer = SwavPeer(cfg, "cpu", dht=dht)
    try:
        assert isinstance(peer.data, ImageFolderMultiCropStream) and len(peer.data.dataset) == 6
        losses = [float(peer.train_step()) for _ in range(2)]
        assert all(math.isfinite(x) for x in losses)
        assert peer.data.num_replaced == 0
    finally:
        peer.shutdown()
        dht.shutdown()


def test_swav_peer_rejects_an_unknown_source(tmp_path):
    from dedloc_amd.training.swav_peer import SwavPeer

    cfg = _tiny_cfg([f"config.CHECKPOINT.DIR={tmp_path}", "config.DATA.TRAIN.DATA_SOURCES=[disk_filelist]"])
    with pytest.raises(ValueError, match="synthetic.*disk_folder"):
        SwavPeer(cfg, "cpu")
    cfg = _tiny_cfg([f"config.CHECKPOINT.DIR={tmp_path}", "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]"])
    with pytest.raises(ValueError, match="DATA_PATHS"):
        SwavPeer(cfg, "cpu")
