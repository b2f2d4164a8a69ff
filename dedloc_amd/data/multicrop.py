"""Synthetic ImageNet + multi-crop SwAV augmentation, generated on the GPU.

Reference pipeline: ``vissl/data/ssl_transforms/img_pil_to_multicrop.py:11-74``
(RandomResizedCrop 2x224 scale (0.14, 1) + 6x96 scale (0.05, 0.14)), RandomHorizontalFlip(0.5),
``img_pil_color_distortion.py`` (ColorJitter(0.8s, 0.8s, 0.8s, 0.2s) with p=0.8, RandomGrayscale
p=0.2), ``img_pil_gaussian_blur.py`` (p=0.5, radius 0.1-2.0), ToTensor, Normalize, and
``collators/multicrop_collator.py:7-55`` (one stacked tensor per crop position).

There is no ImageNet here (no network), so the source images are a fixed pool of smooth random
RGB images generated on the device (``data="synthetic"``).  Every random draw of a batch is made on
the host into one [n*b, 20] parameter table per crop resolution (``MultiCropAugment.sample_params``);
the augmentation itself is ``torch.ops.dedloc.multicrop`` — four HIP kernels per resolution on the
GPU (csrc/kernels/augment.hip: bilinear RandomResizedCrop+flip, colour jitter + grayscale, separable
Gaussian blur, Normalize + bf16 channels-last store) and ``augment_reference`` (plain tensor ops) on
the CPU and as the numerics reference.  The host never decodes or transforms JPEGs.
Real images (``DATA_SOURCES: [disk_folder]``, data/image_folder.py) are decoded on the host and
nothing more: a ragged uint8 batch goes through ``torch.ops.dedloc.multicrop_ragged`` (boxes drawn
in pixels by ``sample_params_ragged``, PIL's area-aware bilinear filter on the GPU) and
``augment_reference_ragged``; colour, blur and normalize are the same code for both sources.
Differences from the PIL path: ColorJitter applies its four ops in a fixed order (torchvision
permutes them) and hue is rotated in YIQ space.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
NP = 20  # parameter-table row, layout in csrc/kernels/augment.hip
_YIQ = torch.tensor([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], dtype=torch.float64)
_LUM = (0.299, 0.587, 0.114)


def _smooth_images(n: int, size: int, gen: torch.Generator, device) -> torch.Tensor:
    """Pool of [n, 3, size, size] images in [0, 1]: multi-octave upsampled noise (natural-ish spectra)."""
    img = torch.zeros(n, 3, size, size, device=device)
    amp = 1.0
    for base in (4, 8, 16, 32, 64):
        noise = torch.rand(n, 3, base, base, generator=gen, device=device)
        img += amp * F.interpolate(noise, size=(size, size), mode="bilinear", align_corners=False)
        amp *= 0.5
    img -= img.amin(dim=(1, 2, 3), keepdim=True)
    img /= img.amax(dim=(1, 2, 3), keepdim=True).clamp_min(1e-6)
    return img


def augment_reference(pool: torch.Tensor, params: torch.Tensor, size: int, rad: int, mean, std) -> torch.Tensor:
    """Tensor-op implementation of ``dedloc::multicrop``: [nb, 3, size, size] bf16, channels-last."""
    prm = params.float()
    nb, dev = prm.shape[0], pool.device
    src = pool.index_select(0, prm[:, 0].long().clamp(0, pool.shape[0] - 1))
    theta = torch.zeros(nb, 2, 3, device=dev)
    theta[:, 0, 0], theta[:, 0, 2], theta[:, 1, 1], theta[:, 1, 2] = prm[:, 1], prm[:, 2], prm[:, 3], prm[:, 4]
    grid = F.affine_grid(theta, [nb, 3, size, size], align_corners=False)
    x = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=False)
    return _color_blur_norm(x, prm, size, rad, mean, std)


def _color_blur_norm(x: torch.Tensor, prm: torch.Tensor, size: int, rad: int, mean, std) -> torch.Tensor:
    """Colour jitter, grayscale, Gaussian blur, Normalize and the bf16 channels-last cast over the
    sampled crops ``x`` [nb, 3, size, size] (table columns 5-19): the tail both sources share."""
    nb, dev = prm.shape[0], x.device
    lum_w = torch.tensor(_LUM, device=dev).view(1, 3, 1, 1)

    def col(k):
        return prm[:, k].view(nb, 1, 1, 1)

    y = x * col(5)                                                                          # brightness
    gm = (y * lum_w).sum(1, keepdim=True).mean(dim=(2, 3), keepdim=True)
    y = (y - gm) * col(6) + gm                                                              # contrast
    g = (y * lum_w).sum(1, keepdim=True)
    y = (y - g) * col(7) + g                                                                # saturation
    y = torch.einsum("bij,bjhw->bihw", prm[:, 10:19].reshape(nb, 3, 3), y).clamp(0, 1)     # hue
    x = torch.where(col(8) != 0, y, x)
    x = torch.where(col(9) != 0, (x * lum_w).sum(1, keepdim=True).expand_as(x), x)          # grayscale
    k = torch.arange(-rad, rad + 1, device=dev, dtype=torch.float32)
    sigma = prm[:, 19]
    ker = torch.exp(-(k.view(1, -1) ** 2) / (2 * sigma.clamp_min(1e-6).view(-1, 1) ** 2))
    ker = ker / ker.sum(1, keepdim=True)
    ident = (k == 0).float().expand_as(ker)
    ker = torch.where((sigma > 0).view(-1, 1), ker, ident).repeat_interleave(3, dim=0)    # [nb*3, 2rad+1]
    x = x.reshape(1, nb * 3, size, size)
    x = F.conv2d(F.pad(x, (rad, rad, 0, 0), mode="reflect"), ker.view(nb * 3, 1, 1, -1), groups=nb * 3)
    x = F.conv2d(F.pad(x, (0, 0, rad, rad), mode="reflect"), ker.view(nb * 3, 1, -1, 1), groups=nb * 3)
    x = x.view(nb, 3, size, size)
    x = (x - torch.tensor(mean, device=dev).view(1, 3, 1, 1)) / torch.tensor(std, device=dev).view(1, 3, 1, 1)
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def crop_resize_ragged(data: torch.Tensor, meta: torch.Tensor, params: torch.Tensor, size: int) -> torch.Tensor:
    """Stage 1 of ``dedloc::multicrop_ragged`` in tensor ops: per table row, crop the box from its
    uint8 HWC image, resize it with the antialiased bilinear filter (PIL's BILINEAR), mirror:
    [nb, 3, size, size] fp32 in [0, 1].  Rows are clamped as the kernel clamps them."""
    prm, nbytes, n = params.float(), data.numel(), meta.shape[0]
    out = []
    for row in prm[:, :5].tolist():
        r = [int(v) if math.isfinite(v) else -10 ** 9 for v in row]
        off, H, W = (int(v) for v in meta[min(max(r[0], 0), n - 1)])
        off = min(max(off, 0), nbytes - 1)
        W = min(max(W, 1), max(nbytes // 3, 1))
        H = min(max(H, 1), max(nbytes // (3 * W), 1))
        w, h = min(max(abs(r[3]), 1), W), min(max(r[4], 1), H)
        j, i = min(max(r[1], 0), W - w), min(max(r[2], 0), H - h)
        idx = (off + torch.arange(H * W * 3, device=data.device)).clamp_(max=nbytes - 1)
        img = data[idx].view(H, W, 3)[i:i + h, j:j + w].permute(2, 0, 1).float().div(255).unsqueeze(0)
        c = F.interpolate(img, size=(size, size), mode="bilinear", antialias=True, align_corners=False)
        out.append(c.flip(3) if row[3] < 0 else c)
    return torch.cat(out)


def augment_reference_ragged(data: torch.Tensor, meta: torch.Tensor, params: torch.Tensor, size: int, rad: int,
                             mean, std) -> torch.Tensor:
    """Tensor-op implementation of ``dedloc::multicrop_ragged``: [nb, 3, size, size] bf16, channels-last."""
    if params.shape[0] == 0:
        return torch.empty(0, 3, size, size, dtype=torch.bfloat16, device=data.device).contiguous(
            memory_format=torch.channels_last)
    return _color_blur_norm(crop_resize_ragged(data, meta, params, size), params.float(), size, rad, mean, std)


class MultiCropAugment:
    def __init__(self, size_crops: Sequence[int] = (224, 96), num_crops: Sequence[int] = (2, 6),
                 crop_scales: Sequence[Tuple[float, float]] = ((0.14, 1.0), (0.05, 0.14)),
                 flip_p: float = 0.5, color_strength: float = 1.0, color_p: float = 0.8, gray_p: float = 0.2,
                 blur_p: float = 0.5, blur_radius: Tuple[float, float] = (0.1, 2.0),
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.size_crops, self.num_crops, self.crop_scales = list(size_crops), list(num_crops), list(crop_scales)
        self.flip_p, self.s, self.color_p, self.gray_p = flip_p, color_strength, color_p, gray_p
        self.blur_p, self.blur_radius = blur_p, blur_radius
        self.mean, self.std = tuple(mean), tuple(std)
        self.rad = int(math.ceil(3 * self.blur_radius[1]))

    def sample_params(self, src: torch.Tensor, scale, gen: torch.Generator) -> torch.Tensor:
        """Host-side draws for one crop resolution: [nb, 20] fp32 table (layout: augment.hip)."""
        nb = src.shape[0]

        def u(lo, hi):
            return torch.empty(nb, dtype=torch.float64).uniform_(lo, hi, generator=gen)

        # RandomResizedCrop(scale, ratio 3/4..4/3) + horizontal flip, normalized coordinates
        area = u(scale[0], scale[1])
        r = torch.exp(u(math.log(3 / 4), math.log(4 / 3)))
        w = torch.sqrt(area * r).clamp(max=1.0)
        h = torch.sqrt(area / r).clamp(max=1.0)
        cx = (torch.rand(nb, dtype=torch.float64, generator=gen) * (1 - w) + w / 2) * 2 - 1
        cy = (torch.rand(nb, dtype=torch.float64, generator=gen) * (1 - h) + h / 2) * 2 - 1
        flip, tail = self._draw_flip_color_blur(nb, gen)
        return torch.cat([torch.stack([src.double(), w * flip, cx, h, cy], 1), tail], 1).float()

    def _draw_flip_color_blur(self, nb: int, gen: torch.Generator):
        """The draws after the geometry, shared by both sources: flip sign [nb] and table columns
        5-19 [nb, 15] (float64)."""
        s = self.s

        def u(lo, hi):
            return torch.empty(nb, dtype=torch.float64).uniform_(lo, hi, generator=gen)

        def coin(p):
            return torch.rand(nb, dtype=torch.float64, generator=gen) < p

        flip = torch.where(coin(self.flip_p), -1.0, 1.0).double()
        lo, hi = max(0.0, 1 - 0.8 * s), 1 + 0.8 * s
        bright, contrast, sat = u(lo, hi), u(lo, hi), u(lo, hi)
        hue = u(-0.2 * s, 0.2 * s) * (2 * math.pi)
        apply, grey = coin(self.color_p).double(), coin(self.gray_p).double()
        sigma = u(*self.blur_radius)
        sigma = torch.where(coin(self.blur_p), sigma, torch.zeros_like(sigma))
        # hue: rotate the I/Q chroma plane of YIQ, folded into one RGB->RGB matrix per image
        rot = torch.zeros(nb, 3, 3, dtype=torch.float64)
        rot[:, 0, 0] = 1
        rot[:, 1, 1], rot[:, 1, 2], rot[:, 2, 1], rot[:, 2, 2] = hue.cos(), -hue.sin(), hue.sin(), hue.cos()
        M = torch.linalg.inv(_YIQ) @ rot @ _YIQ
        t = torch.stack([bright, contrast, sat, apply, grey], 1)
        return flip, torch.cat([t, M.reshape(nb, 9), sigma.view(-1, 1)], 1)

    @staticmethod
    def _rrc_box(H: torch.Tensor, W: torch.Tensor, scale, gen: torch.Generator):
        """torchvision's ``RandomResizedCrop.get_params`` (ratio 3/4..4/3), vectorised over images of
        heights ``H`` and widths ``W``: ten attempts, the first that fits wins, else the centred box
        with its ratio clamped.  Returns float64 (left, top, width, height) in pixels."""
        nb = H.shape[0]
        Hd, Wd = H.double(), W.double()
        tries = 10
        area = torch.empty(nb, tries, dtype=torch.float64).uniform_(scale[0], scale[1], generator=gen) * (Hd * Wd)[:, None]
        r = torch.exp(torch.empty(nb, tries, dtype=torch.float64).uniform_(math.log(3 / 4), math.log(4 / 3),
                                                                           generator=gen))
        w = torch.round(torch.sqrt(area * r))
        h = torch.round(torch.sqrt(area / r))
        ok = (w > 0) & (w <= Wd[:, None]) & (h > 0) & (h <= Hd[:, None])
        first = ok.double().argmax(1, keepdim=True)  # the first fitting attempt (0 when none fits)
        w, h, fits = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0], ok.any(1)
        # fallback: the whole image, cut to the nearest ratio in [3/4, 4/3], centred
        ratio = Wd / Hd
        fw = torch.where(ratio > 4 / 3, torch.round(Hd * (4 / 3)), Wd)
        fh = torch.where(ratio < 3 / 4, torch.round(Wd / (3 / 4)), Hd)
        ui, uj = (torch.rand(nb, dtype=torch.float64, generator=gen) for _ in range(2))
        w, h = torch.where(fits, w, fw), torch.where(fits, h, fh)
        i = torch.where(fits, torch.floor(ui * (Hd - h + 1)).clamp(max=Hd - h), torch.floor((Hd - h) / 2))
        j = torch.where(fits, torch.floor(uj * (Wd - w + 1)).clamp(max=Wd - w), torch.floor((Wd - w) / 2))
        return j, i, w, h

    def sample_params_ragged(self, src: torch.Tensor, H: torch.Tensor, W: torch.Tensor, scale,
                             gen: torch.Generator) -> torch.Tensor:
        """Host-side draws for one crop resolution over images of different sizes ([nb] rows ``src``
        of the batch's image table, their heights ``H`` and widths ``W``): [nb, 20] fp32 table for
        ``dedloc::multicrop_ragged`` (columns 0-4: row, box left, top, width (negative: mirrored),
        height, in pixels).  The box is ``_rrc_box``."""
        j, i, w, h = self._rrc_box(H, W, scale, gen)
        flip, tail = self._draw_flip_color_blur(src.shape[0], gen)
        return torch.cat([torch.stack([src.double(), j, i, w * flip, h], 1), tail], 1).float()

    @classmethod
    def crop_flip_params(cls, src: torch.Tensor, H: torch.Tensor, W: torch.Tensor, gen: torch.Generator,
                         scale=(0.08, 1.0), flip_p: float = 0.5) -> torch.Tensor:
        """The linear-evaluation train transform ``RandomResizedCrop(scale, ratio 3/4..4/3)`` +
        ``RandomHorizontalFlip(flip_p)`` as a [nb, 20] table for ``dedloc::multicrop_ragged``: the
        box of ``_rrc_box``, the mirror in the width's sign, and the colour and blur columns at
        identity as in ``center_params``."""
        j, i, w, h = cls._rrc_box(H, W, scale, gen)
        flip = torch.where(torch.rand(src.shape[0], dtype=torch.float64, generator=gen) < flip_p, -1.0, 1.0).double()
        p = torch.zeros(src.shape[0], 20, dtype=torch.float64)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4] = src.double(), j, i, w * flip, h
        p[:, 5:8] = 1.0
        p[:, 10], p[:, 14], p[:, 18] = 1.0, 1.0, 1.0
        return p.float()

    @staticmethod
    def center_params(src: torch.Tensor, H: torch.Tensor, W: torch.Tensor, size: int, resize: int) -> torch.Tensor:
        """The evaluation transform ``Resize(resize)`` + ``CenterCrop(size)`` as a [n, 20] table for
        ``dedloc::multicrop_ragged``: the centred square box of side
        max(1, round(min(H, W) * size / resize)) (at most the image's shorter side), which the
        sampler resizes to ``size`` with the same area-aware bilinear filter; no mirror, and the
        colour columns at identity (brightness, contrast, saturation 1, apply 0, grey 0, identity
        hue matrix, sigma 0).  One difference from resizing first and cropping after: the filter's
        taps at the box edge do not see the pixels outside the box."""
        Hd, Wd = H.double(), W.double()
        short = torch.minimum(Hd, Wd)
        side = torch.floor(short * size / resize + 0.5).clamp(min=1.0)
        side = torch.minimum(side, short)
        j, i = torch.floor((Wd - side) / 2), torch.floor((Hd - side) / 2)
        p = torch.zeros(src.shape[0], 20, dtype=torch.float64)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4] = src.double(), j, i, side, side
        p[:, 5:8] = 1.0
        p[:, 10], p[:, 14], p[:, 18] = 1.0, 1.0, 1.0
        return p.float()

    @torch.no_grad()
    def ragged(self, data: torch.Tensor, meta: torch.Tensor, H: torch.Tensor, W: torch.Tensor, gen: torch.Generator,
               out_dtype=torch.bfloat16) -> List[torch.Tensor]:
        """Multi-crop of a ragged uint8 batch (``data`` / ``meta`` on the device, layout in
        augment.hip; ``H``, ``W``: the same sizes on the host): one [b, 3, s, s] channels-last tensor
        per crop."""
        import dedloc_amd.ops  # noqa: F401  (registers dedloc::multicrop_ragged)

        b = meta.shape[0]
        src = torch.arange(b)
        crops = []
        for size, n, scale in zip(self.size_crops, self.num_crops, self.crop_scales):
            params = self.sample_params_ragged(src.repeat(n), H.repeat(n), W.repeat(n), scale, gen)
            if data.is_cuda:
                params = params.pin_memory().to(data.device, non_blocking=True)
            x = torch.ops.dedloc.multicrop_ragged(data, meta, params, size, self.rad, list(self.mean), list(self.std))
            if x.dtype != out_dtype:
                x = x.to(out_dtype)
            crops.extend(x.split(b))
        return crops

    @torch.no_grad()
    def __call__(self, pool: torch.Tensor, src: torch.Tensor, gen: torch.Generator,
                 out_dtype=torch.bfloat16) -> List[torch.Tensor]:
        """``src``: [b] host indices into ``pool``; one [b, 3, s, s] channels-last tensor per crop."""
        import dedloc_amd.ops  # noqa: F401  (registers dedloc::multicrop)

        b = src.shape[0]
        crops = []
        for size, n, scale in zip(self.size_crops, self.num_crops, self.crop_scales):
            # all n crops of one resolution in one batched pass over n*b images
            params = self.sample_params(src.repeat(n), scale, gen)
            if pool.is_cuda:
                params = params.pin_memory().to(pool.device, non_blocking=True)
            x = torch.ops.dedloc.multicrop(pool, params, size, self.rad, list(self.mean), list(self.std))
            if x.dtype != out_dtype:
                x = x.to(out_dtype)
            crops.extend(x.split(b))
        return crops


class SyntheticMultiCropStream:
    """Per-peer stream of multi-crop batches drawn from a device-resident synthetic image pool."""

    def __init__(self, batch_size: int, device, seed: int = 0, pool_size: int = 1024, image_size: int = 256,
                 augment: MultiCropAugment = None, out_dtype=torch.bfloat16):
        self.batch_size, self.device = batch_size, torch.device(device)
        pool_gen = torch.Generator(device=self.device)
        pool_gen.manual_seed(seed)
        self.pool = _smooth_images(pool_size, image_size, pool_gen, self.device)
        self.gen = torch.Generator().manual_seed(seed)  # host draws: source images, geometry, colour, blur
        self.augment = augment or MultiCropAugment()
        self.out_dtype = out_dtype

    def next_batch(self) -> List[torch.Tensor]:
        idx = torch.randint(0, self.pool.shape[0], (self.batch_size,), generator=self.gen)
        return self.augment(self.pool, idx, self.gen, self.out_dtype)


class StreamPrefetcher:
    """Overlaps batch generation with training: while the caller's stream computes on batch i,
    batch i+1 is produced on a side stream (the reference's DataLoader workers prepare batches
    ahead on the CPU; here the augmentation kernels run ahead on the GPU).  ``next_batch`` makes the
    caller's stream wait for the batch it returns and records that stream on its tensors, so the
    caching allocator never hands their memory to the side stream while the caller still reads it."""

    def __init__(self, source, device):
        self.source = source
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self._next = None

    def _launch(self):
        with torch.cuda.stream(self.stream):
            batch = self.source.next_batch()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._next = (batch, ev)

    def next_batch(self) -> List[torch.Tensor]:
        if self.stream is None:
            return self.source.next_batch()
        if self._next is None:
            self._launch()
        batch, ev = self._next
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in batch:
            t.record_stream(cur)
        self._launch()  # the following batch, under this iteration's compute
        return batch

    def __getattr__(self, name):  # pool, batch_size, augment, ... of the wrapped stream
        if name == "source":  # not set yet (copy / unpickle): no recursion through __getattr__
            raise AttributeError(name)
        return getattr(self.source, name)
