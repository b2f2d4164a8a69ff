"""Real images for SwAV: vissl's ``disk_folder`` source (``vissl/data/disk_dataset.py``) feeding the
GPU multi-crop pipeline.

The host only decodes.  A batch of decoded uint8 HWC images of different sizes is packed back to
back into one pinned buffer behind its [n, 3] int64 table of (byte offset, H, W), sent to the
device with one non-blocking copy, and every transform of the reference's PIL pipeline
(RandomResizedCrop with PIL's area-aware bilinear filter, flip, colour, blur, normalize) runs there
in ``torch.ops.dedloc.multicrop_ragged`` (csrc/kernels/augment.hip).  Decoding runs in a thread pool
(threads, never processes: nothing else opens the GPU) a few batches ahead of the consumer.

``ImageFolderEvalStream`` is the labelled, unshuffled view of the same directories for evaluation
(``training/swav_eval.py``): every image once, under Resize + CenterCrop through the same sampler.
``ImageFolderLabelledStream`` is the labelled, per-epoch reshuffled training view for the linear
evaluation (``training/swav_linear.py``): RandomResizedCrop + flip, no colour or blur.

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
    ``paths``.  ``classes`` are the sorted names of the first-level sub-directories of the roots
    (torchvision ``ImageFolder``'s rule, which vissl's ``disk_folder`` label source uses) and
    ``labels`` [len(files)] int64 holds, aligned with ``files``, the class index of each file's
    first-level sub-directory (-1 for a file directly under a root); training ignores them.
    ``load(i)`` returns a contiguous uint8 [H, W, 3] RGB array whose longer side is at most
    ``max_image_side``."""

    def __init__(self, paths: Sequence[str], max_image_side: int = 512):
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        self.max_image_side = int(max_image_side)
        self._image = _pil()  # imported once, lazily with the first dataset; None without PIL
        exts = (IMAGE_EXTENSIONS if self._image is not None else ()) + (".npy",)
        files, class_of, classes = [], {}, set()
        for root in paths:
            if not os.path.isdir(root):
                raise FileNotFoundError(f"DATA_PATHS entry {root!r} is not a directory")
            classes.update(e.name for e in os.scandir(root) if e.is_dir())
            for d, _, names in os.walk(root, followlinks=True):
                rel = os.path.relpath(d, root)
                top = None if rel == os.curdir else rel.split(os.sep)[0]
                for n in names:
                    if n.lower().endswith(exts):
                        files.append(os.path.join(d, n))
                        class_of[files[-1]] = top
        self.files: List[str] = sorted(files)
        self.classes: List[str] = sorted(classes)
        index = {c: i for i, c in enumerate(self.classes)}
        self.labels = torch.tensor([index.get(class_of[f], -1) for f in self.files], dtype=torch.int64)
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


class _RaggedBatcher:
    """What the image-folder streams share: the decode thread pool, the ring of pinned staging
    buffers, and the packing of one batch of decoded images into the ragged device buffer of
    ``dedloc::multicrop_ragged``."""

    def __init__(self, device, dataset: ImageFolderDataset, num_workers: int, ring: int):
        self.device = torch.device(device)
        self.dataset = dataset
        self.num_workers = max(1, min(int(num_workers), MAX_WORKERS))
        self._pool = ThreadPoolExecutor(self.num_workers, thread_name_prefix="image_decode")
        # ring of pinned staging buffers: [buffer, event recorded after its last copy]
        self._ring = [[None, None] for _ in range(max(2, ring))]
        self._slot = 0

    @property
    def num_replaced(self) -> int:
        return self.dataset.num_replaced

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

    def _pack(self, imgs):
        """Decoded uint8 HWC images -> (data, meta) on the device (layout: augment.hip) and their
        heights and widths on the host."""
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
        return dev[head:], dev[:head].view(torch.int64).view(n, 3), H, W

    def close(self):
        self._pool.shutdown(wait=False, cancel_futures=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class ImageFolderMultiCropStream(_RaggedBatcher):
    """Per-peer stream of multi-crop batches from an image directory, with the interface of
    ``SyntheticMultiCropStream``.  Each peer draws its own permutation of the dataset from its seed
    and reshuffles it every epoch, so every image is served once per epoch (a dataset smaller than
    a batch wraps into the next epoch's permutation)."""

    def __init__(self, batch_size: int, device, dataset: ImageFolderDataset, seed: int = 0,
                 augment: MultiCropAugment = None, out_dtype=torch.bfloat16, num_workers: int = 8,
                 prefetch_batches: int = 2):
        self.prefetch_batches = max(0, int(prefetch_batches))
        super().__init__(device, dataset, num_workers, self.prefetch_batches)
        self.batch_size = batch_size
        self.augment = augment or MultiCropAugment()
        self.out_dtype = out_dtype
        self.gen = torch.Generator().manual_seed(seed)        # host draws: geometry, colour, blur
        self.order_gen = torch.Generator().manual_seed(seed)  # epoch permutations (drawn ahead of the batches)
        self._order: deque = deque()    # indices of the current permutation not yet submitted
        self._pending: deque = deque()  # batches being decoded: lists of futures

    def _submit(self):
        futs = []
        for _ in range(self.batch_size):
            if not self._order:
                self._order.extend(torch.randperm(len(self.dataset), generator=self.order_gen).tolist())
            futs.append(self._pool.submit(self.dataset.load, self._order.popleft()))
        self._pending.append(futs)

    def next_batch(self) -> List[torch.Tensor]:
        while len(self._pending) < self.prefetch_batches + 1:
            self._submit()
        imgs = [f.result() for f in self._pending.popleft()]
        self._submit()  # keep the decoders prefetch_batches ahead
        data, meta, H, W = self._pack(imgs)
        return self.augment.ragged(data, meta, H, W, self.gen, self.out_dtype)


class ImageFolderEvalStream(_RaggedBatcher):
    """The evaluation view of an image directory: the images ``indices`` (default: all) in that
    order, once each, unshuffled, under the deterministic transform ``Resize(resize)`` +
    ``CenterCrop(size)`` + Normalize (``MultiCropAugment.center_params`` through the ragged GPU
    sampler).  Iterating yields ``(images [b, 3, size, size] bf16 channels-last, labels [b] int64)``
    on the device; the last batch is short.  Every iteration starts from the first image."""

    def __init__(self, dataset: ImageFolderDataset, batch_size: int, device, indices=None, size: int = 224,
                 resize: int = 256, num_workers: int = 8, prefetch_batches: int = 2):
        self.prefetch_batches = max(0, int(prefetch_batches))
        super().__init__(device, dataset, num_workers, self.prefetch_batches)
        self.batch_size, self.size, self.resize = int(batch_size), int(size), int(resize)
        self.indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
        self.labels = dataset.labels[self.indices]
        self.augment = MultiCropAugment()  # mean / std of the training pipeline; no random draw is used

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        import dedloc_amd.ops  # noqa: F401  (registers dedloc::multicrop_ragged)

        B, aug = self.batch_size, self.augment
        starts = list(range(0, len(self.indices), B))
        pending: deque = deque()
        nxt = 0
        for s in starts:
            while nxt < len(starts) and len(pending) < self.prefetch_batches + 1:
                chunk = self.indices[starts[nxt]:starts[nxt] + B]
                pending.append([self._pool.submit(self.dataset.load, i) for i in chunk])
                nxt += 1
            imgs = [f.result() for f in pending.popleft()]
            data, meta, H, W = self._pack(imgs)
            params = aug.center_params(torch.arange(len(imgs)), H, W, self.size, self.resize)
            labels = self.labels[s:s + B]
            if data.is_cuda:
                params = params.pin_memory().to(data.device, non_blocking=True)
                labels = labels.pin_memory().to(data.device, non_blocking=True)
            x = torch.ops.dedloc.multicrop_ragged(data, meta, params, self.size, aug.rad, list(aug.mean), list(aug.std))
            yield x, labels


class ImageFolderLabelledStream(_RaggedBatcher):
    """The labelled training view of an image directory for the linear evaluation
    (``training/swav_linear.py``): the images ``indices`` (default: all) in a fresh fixed-seed
    permutation per epoch, each under a fresh ``RandomResizedCrop(size)`` + ``RandomHorizontalFlip`` +
    Normalize (``MultiCropAugment.crop_flip_params`` through the ragged GPU sampler).
    ``epoch(e)`` yields ``(images [b, 3, size, size] bf16 channels-last, labels [b] int64)`` on the
    device; the last batch of an epoch is short.  Epoch ``e``'s order and crops depend on ``seed``
    and ``e`` only."""

    def __init__(self, dataset: ImageFolderDataset, batch_size: int, device, indices=None, labels=None,
                 size: int = 224, seed: int = 0, num_workers: int = 8, prefetch_batches: int = 2):
        self.prefetch_batches = max(0, int(prefetch_batches))
        super().__init__(device, dataset, num_workers, self.prefetch_batches)
        self.batch_size, self.size, self.seed = int(batch_size), int(size), int(seed)
        self.indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
        self.labels = dataset.labels[self.indices] if labels is None else labels
        self.augment = MultiCropAugment()  # mean / std of the training pipeline

    def __len__(self):
        return len(self.indices)

    def steps_per_epoch(self) -> int:
        return -(-len(self.indices) // self.batch_size)

    def epoch(self, e: int):
        import dedloc_amd.ops  # noqa: F401  (registers dedloc::multicrop_ragged)

        B, aug = self.batch_size, self.augment
        gen = torch.Generator().manual_seed(self.seed + 7919 * int(e))
        order = torch.randperm(len(self.indices), generator=gen).tolist()
        starts = list(range(0, len(order), B))
        pending: deque = deque()
        nxt = 0
        for s in starts:
            while nxt < len(starts) and len(pending) < self.prefetch_batches + 1:
                chunk = order[starts[nxt]:starts[nxt] + B]
                pending.append([self._pool.submit(self.dataset.load, self.indices[k]) for k in chunk])
                nxt += 1
            imgs = [f.result() for f in pending.popleft()]
            data, meta, H, W = self._pack(imgs)
            params = aug.crop_flip_params(torch.arange(len(imgs)), H, W, gen)
            labels = self.labels[order[s:s + B]]
            if data.is_cuda:
                params = params.pin_memory().to(data.device, non_blocking=True)
                labels = labels.pin_memory().to(data.device, non_blocking=True)
            x = torch.ops.dedloc.multicrop_ragged(data, meta, params, self.size, aug.rad, list(aug.mean), list(aug.std))
            yield x, labels
