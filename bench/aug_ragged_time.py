"""The disk_folder SwAV source, measured: prints one JSON line per measurement.

  op      GPU ms per batch of 64 (2x224 + 6x96 crops) of dedloc::multicrop_ragged on 375x500 uint8
          images, beside the synthetic dedloc::multicrop (bench/aug_time.py) in the same process
  decode  host decode rate (images/s) of 375x500 JPEGs at 1, 4, 8 and 16 threads, and of .npy files
  peer    the PerfStats `data` phase and samples/s over 30 SwavPeer iterations at b=64 with
          disk_folder (JPEG and .npy folders) against synthetic

    python bench/aug_ragged_time.py [op] [decode] [peer] [--out FILE]
"""
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderMultiCropStream  # noqa: E402
from dedloc_amd.data.multicrop import SyntheticMultiCropStream, _smooth_images  # noqa: E402

H, W = 375, 500
OUT = None


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def write_folder(root, n, kind):
    """n natural-ish 375x500 images (multi-octave noise: JPEG sizes and decode cost near a photo's)."""
    img = _smooth_images(32, 512, torch.Generator().manual_seed(0), "cpu")[:, :, :H, :W]  # 32 distinct images
    arr = (img * 255).round().byte().permute(0, 2, 3, 1).contiguous().numpy()
    os.makedirs(root, exist_ok=True)
    for k in range(n):
        if kind == "npy":
            np.save(os.path.join(root, f"{k:04d}.npy"), arr[k % 32])
        else:
            from PIL import Image

            Image.fromarray(arr[k % 32]).save(os.path.join(root, f"{k:04d}.jpg"), quality=90)
    return root


def time_stream(s, calls=20):
    for _ in range(3):
        s.next_batch()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(calls):
        s.next_batch()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / calls, (time.perf_counter() - t0) * 1e3 / calls


def bench_op(tmp):
    dev = torch.device("cuda")
    syn = SyntheticMultiCropStream(64, dev)
    rag = ImageFolderMultiCropStream(64, dev, ImageFolderDataset([write_folder(tmp + "/op_npy", 128, "npy")]),
                                     num_workers=8)
    aug = rag.augment
    # the op alone: one resident ragged batch, fresh host draws per call as in the synthetic stream
    imgs = [rag.dataset.load(k) for k in range(64)]
    data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    hw = torch.tensor([[a.shape[0], a.shape[1]] for a in imgs])
    sizes = hw[:, 0] * hw[:, 1] * 3
    meta = torch.stack([torch.cumsum(sizes, 0) - sizes, hw[:, 0], hw[:, 1]], 1).to(dev)

    class Resident:
        def next_batch(self):
            return aug.ragged(data, meta, hw[:, 0], hw[:, 1], rag.gen)

    for rep in range(2):  # alternate the two sources: same process, same clocks
        ms, wall = time_stream(syn)
        emit(bench="aug_op", source="synthetic", rep=rep, batch=64, gpu_ms_per_batch=round(ms, 4),
             wall_ms_per_batch=round(wall, 4))
        ms, wall = time_stream(Resident())
        emit(bench="aug_op", source="ragged_resident_375x500", rep=rep, batch=64, gpu_ms_per_batch=round(ms, 4),
             wall_ms_per_batch=round(wall, 4))
        ms, wall = time_stream(rag)
        emit(bench="aug_op", source="disk_folder_npy_stream_375x500", rep=rep, batch=64,
             gpu_ms_per_batch=round(ms, 4), wall_ms_per_batch=round(wall, 4))
    rag.close()


def bench_decode(tmp):
    for kind, n in (("jpg", 256), ("npy", 256)):
        ds = ImageFolderDataset([write_folder(f"{tmp}/dec_{kind}", n, kind)])
        for threads in (1, 4, 8, 16):
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(ds.load, range(min(n, 32))))  # page cache, decoder warm-up
                t0 = time.perf_counter()
                for _ in range(3):
                    list(ex.map(ds.load, range(n)))
                dt = time.perf_counter() - t0
            emit(bench="decode", kind=kind, image=f"{H}x{W}", threads=threads, images_per_s=round(3 * n / dt, 1))


def bench_peer(tmp):
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer
    from dedloc_amd.utils.config import load_config

    folders = {"synthetic": None, "disk_folder_jpg": write_folder(tmp + "/peer_jpg", 512, "jpg"),
               "disk_folder_npy": write_folder(tmp + "/peer_npy", 512, "npy")}
    for name, root in folders.items():
        ov = ["config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=64", "config.LOG_FREQUENCY=1", f"config.CHECKPOINT.DIR={tmp}",
              "config.CHECKPOINT.AUTO_RESUME=false"]
        if root:
            ov += ["config.DATA.TRAIN.DATA_SOURCES=[disk_folder]", f"+config.DATA.TRAIN.DATA_PATHS=[{root}]",
                   "config.DATA.TRAIN.NUM_DATALOADER_WORKERS=16"]
        dht = DHT(start=True)
        peer = SwavPeer(load_config("swav_1node_resnet_submit", ov), torch.device("cuda"), dht=dht)
        try:
            for _ in range(8):  # eager warm-up, graph capture, first replays
                peer.train_step()
            torch.cuda.synchronize()
            peer.perf.report(block=True)
            t0 = time.perf_counter()
            for _ in range(30):
                peer.train_step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rep = peer.perf.report(block=True)
            emit(bench="swav_peer_data_phase", source=name, batch=64, iterations=30,
                 samples_per_s=round(30 * 64 / dt, 1), **{k: round(v, 3) for k, v in rep.items()})
        finally:
            peer.shutdown()
            dht.shutdown()


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        OUT = args[args.index("--out") + 1]
        args = [a for a in args if a not in ("--out", OUT)]
    which = args or ["op", "decode", "peer"]
    assert torch.cuda.is_available() or which == ["decode"], "op and peer measure the GPU"
    with tempfile.TemporaryDirectory() as tmp:
        for w in which:
            {"op": bench_op, "decode": bench_decode, "peer": bench_peer}[w](tmp)
