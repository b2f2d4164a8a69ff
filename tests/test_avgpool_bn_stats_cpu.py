"""The CPU implementation of ops.avgpool_bn_stats (the reference the GPU test's shapes are pinned on)
against torch's avg_pool2d in float64 followed by the per-channel sum and sum of squares."""
import pytest
import torch

import dedloc_amd.ops as ops

# (N, H, W, C, k, stride, pad): the GPU test's shapes (tests/test_avgpool_bn_stats_gpu.py)
SHAPES = [(2, 12, 12, 64, 10, 10, 4), (1, 24, 24, 64, 16, 8, 0), (2, 18, 18, 72, 13, 5, 0), (3, 7, 7, 2048, 6, 1, 0),
          (1, 6, 6, 8, 6, 1, 0), (2, 11, 9, 64, 3, 2, 1)]


def make_input(shape, device="cpu"):
    N, H, W, C = shape[:4]
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(H * W + C)) * 2 + 0.5
    return x.bfloat16().to(device).contiguous(memory_format=torch.channels_last)


def reference(x, k, s, p):
    """float64: pooled values, their per-channel sum and sum of squares, and sum |x| over each window / k^2."""
    xd = x.double().cpu()
    y = torch.nn.functional.avg_pool2d(xd, k, s, p)
    return y, y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3)), torch.nn.functional.avg_pool2d(xd.abs(), k, s, p)


def check(shape, device):
    k, s, p = shape[4:]
    x = make_input(shape, device)
    y, s1, s2 = ops.avgpool_bn_stats(x, k, s, p)
    want, w1, w2, mag = reference(x, k, s, p)
    assert y.shape == want.shape and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    assert s1.dtype == s2.dtype == torch.float32 and s1.shape == s2.shape == (shape[3],)
    # y is fp32: the fp32 accumulation of at most 256 exact bf16 terms
    err = (y.double().cpu() - want).abs()
    bound = 2.0 ** -20 * mag
    e1 = ((s1.double().cpu() - w1).norm() / w1.norm()).item()
    e2 = ((s2.double().cpu() - w2).norm() / w2.norm()).item()
    print(f"avgpool_bn_stats {device} {shape}: max err/bound {(err / bound.clamp_min(1e-30)).max().item():.3f}, "
          f"sum rel {e1:.2e}, sumsq rel {e2:.2e}")
    assert (err <= bound).all()
    assert e1 <= 1e-5 and e2 <= 1e-5
    return y, s1, s2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_reference_matches_float64_avg_pool2d(shape):
    check(shape, "cpu")
