"""Real images for SwAV: vissl's ``disk_folder`` source (``vissl/data/disk_dataset.py``) feeding the
GPU multi-crop pipeline.

The host only decodes.  A batch of decoded uint8 HWC images of different sizes is packed back to
back into one pinned buffer behind its [n, 3] int64 table of (byte offset, H, W), sent to the
device with one non-blocking copy, and every transform of the reference's PIL pipeline
(RandomResizedCrop with PIL's area-aware bilinear filter, flip, colour, blur, normalize) runs there
in ``torch.ops.dedloc.multicrop_ragged`` (csrc/kernels/augment.hip).  Decoding runs in a thread pool
(threads, never processes: nothing else opens the GPU) a few batches ahead of the consumer.

Besides image files the dataset serves ``.npy`` files holding a uint8 [H, W, 3] array: a
pre-decoded form that needs no PIL and no JPEG decode.
"""
from __future__ import annotations

import logging
import os
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence

import numpy as np
import torch

from .multicrop import MultiCropAugment

logger = logging.getLogger(__name__)

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".ppm")
GRAY_IMAGE_SIZE = 224  # vissl DATA.TRAIN.DEFAULT_GRAY_IMG_SIZE: what an unreadable file becomes
MAX_WORKERS = 16


def _pil():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


class ImageFolderDataset:
    """Sorted recursive listing of the image files (and ``.npy`` uint8 [H, W, 3] arrays) under
    ``paths``; class sub-directories are walked, labels ignored.  ``load(i)`` returns a contiguous
    uint8 [H, W, 3] RGB array whose longer side is at most ``max_image_side``."""

    def __init__(self, paths: Sequence[str], max_image_side: int = 512):
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        self.max_image_side = int(max_image_side)
        self._image = _pil()  # imported once, lazily with the first dataset; None without PIL
        exts = (IMAGE_EXTENSIONS if self._image is not None else ()) + (".npy",)
        files = []
        for root in paths:
            if not os.path.isdir(root):
                raise FileNotFoundError(f"DATA_PATHS entry {root!r} is not a directory")
            for d, _, names in os.walk(root, followlinks=True):
                files.extend(os.path.join(d, n) for n in names if n.lower().endswith(exts))
        self.files: List[str] = sorted(files)
        if not self.files:
            hint = "" if self._image is not None else \
                " (PIL is not installed: only .npy files holding uint8 [H, W, 3] arrays are served)"
            raise FileNotFoundError(f"no images under {list(paths)}{hint}")
        self.num_replaced = 0  # unreadable files served as the grey image (counted per load)
        self._bad = set()
        self._lock = threading.Lock()

    def __len__(self):
        return len(self.files)

    def _shrink(self, arr: np.ndarray) -> np.ndarray:
        H, W = arr.shape[:2]
        m = self.max_image_side
        if m <= 0 or max(H, W) <= m:
            return arr
        nh, nw = max(1, round(H * m / max(H, W))), max(1, round(W * m / max(H, W)))
        if self._image is not None:
            return np.asarray(self._image.fromarray(arr).resize((nw, nh), self._image.BILINEAR))
        import torch.nn.functional as F

        t = torch.from_numpy(arr).permute(2, 0, 1).unsqueeze(0).float()
        t = F.interpolate(t, size=(nh, nw), mode="bilinear", antialias=True, align_corners=False)
        return t.round_().clamp_(0, 255).byte()[0].permute(1, 2, 0).contiguous().numpy()

    def _decode(self, path: str) -> np.ndarray:
        if path.lower().endswith(".npy"):
            arr = np.load(path, allow_pickle=False)
            if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3 or arr.size == 0:
                raise ValueError(f"expected a uint8 [H, W, 3] array, got {arr.dtype} {arr.shape}")
            return self._shrink(arr)
        with self._image.open(path) as img:
            m = self.max_image_side
            if m > 0 and max(img.size) > m:
                img.draft("RGB", (m, m))  # JPEG: decode at 1/2, 1/4, 1/8 scale, still >= the target
            arr = np.asarray(img.convert("RGB"))
        return self._shrink(arr)

    def load(self, index: int) -> np.ndarray:
        path = self.files[index]
        try:
            return np.ascontiguousarray(self._decode(path))
        except Exception as e:  # noqa: BLE001  (any decoder error: vissl serves the grey image)
            with self._lock:
                self.num_replaced += 1
                if path not in self._bad:
                    self._bad.add(path)
                    logger.warning(f"unreadable image {path} ({e!r}): replaced by a grey image")
            return np.full((GRAY_IMAGE_SIZE, GRAY_IMAGE_SIZE, 3), 128, dtype=np.uint8)


class ImageFolderMultiCropStream:
    """Per-peer stream of multi-crop batches from an image directory, with the interface of
    ``SyntheticMultiCropStream``.  Each peer draws its own permutation of the dataset from its seed
    and reshuffles it every epoch, so every image is served once per epoch (a dataset smaller than
    a batch wraps into the next epoch's permutation)."""

    def __init__(self, batch_size: int, device, dataset: ImageFolderDataset, seed: int = 0,
                 augment: MultiCropAugment = None, out_dtype=torch.bfloat16, num_workers: int = 8,
                 prefetch_batches: int = 2):
        self.batch_size, self.device = batch_size, torch.device(device)
        self.dataset = dataset
        self.augment = augment or MultiCropAugment()
        self.out_dtype = out_dtype
        self.gen = torch.Generator().manual_seed(seed)        # host draws: geometry, colour, blur
        self.order_gen = torch.Generator().manual_seed(seed)  # epoch permutations (drawn ahead of the batches)
        self.num_workers = max(1, min(int(num_workers), MAX_WORKERS))
        self.prefetch_batches = max(0, int(prefetch_batches))
        self._pool = ThreadPoolExecutor(self.num_workers, thread_name_prefix="image_decode")
        self._order: deque = deque()    # indices of the current permutation not yet submitted
        self._pending: deque = deque()  # batches being decoded: lists of futures
        # ring of pinned staging buffers: [buffer, event recorded after its last copy]
        self._ring = [[None, None] for _ in range(max(2, self.prefetch_batches))]
        self._slot = 0

    @property
    def num_replaced(self) -> int:
        return self.dataset.num_replaced

    def _submit(self):
        futs = []
        for _ in range(self.batch_size):
            if not self._order:
                self._order.extend(torch.randperm(len(self.dataset), generator=self.order_gen).tolist())
            futs.append(self._pool.submit(self.dataset.load, self._order.popleft()))
        self._pending.append(futs)

    def _staging(self, nbytes: int) -> torch.Tensor:
        """The next pinned buffer of the ring (a plain host tensor on a CPU device), at least
        ``nbytes`` long and no longer read by the copy that last used it."""
        slot = self._ring[self._slot]
        self._slot = (self._slot + 1) % len(self._ring)
        buf, ev = slot
        if ev is not None:
            ev.synchronize()  # this buffer's copy only: never a device-wide synchronise
            slot[1] = None
        if buf is None or buf.numel() < nbytes:
            cap = -(-nbytes * 5 // 4 // 4096) * 4096
            buf = slot[0] = torch.empty(cap, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        return slot

    def next_batch(self) -> List[torch.Tensor]:
        while len(self._pending) < self.prefetch_batches + 1:
            self._submit()
        imgs = [f.result() for f in self._pending.popleft()]
        self._submit()  # keep the decoders prefetch_batches ahead
        n = len(imgs)
        H = torch.tensor([a.shape[0] for a in imgs], dtype=torch.int64)
        W = torch.tensor([a.shape[1] for a in imgs], dtype=torch.int64)
        sizes = H * W * 3
        off = torch.cumsum(sizes, 0) - sizes
        head = n * 24  # the int64 [n, 3] table leads the buffer, the images follow back to back
        total = head + int(sizes.sum())
        slot = self._staging(total)
        buf = slot[0]
        buf[:head].view(torch.int64).view(n, 3).copy_(torch.stack([off, H, W], 1))
        host = buf.numpy()
        for a, o in zip(imgs, off.tolist()):
            host[head + o: head + o + a.size] = a.reshape(-1)
        if self.device.type == "cuda":
            dev = buf[:total].to(self.device, non_blocking=True)  # one copy, on the current stream
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            slot[1] = ev
        else:
            dev = buf[:total].clone()
        meta, data = dev[:head].view(torch.int64).view(n, 3), dev[head:]
        return self.augment.ragged(data, meta, H, W, self.gen, self.out_dtype)

    def close(self):
        self._pool.shutdown(wait=False, cancel_futures=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass
