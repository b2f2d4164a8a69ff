"""The pool_eval.hip kernels (ops.avgpool_bn_stats on the GPU) against a float64 torch reference on the
same bf16 inputs, at the smallest shapes where each mechanism can break: padding and zero taps in
the divisor, windows across strip seams, a channel-slab tail, uncovered trailing rows / columns,
several slabs and strips, one output pixel, a non-square input."""
import pytest
import torch

import dedloc_amd.ops as ops
from test_avgpool_bn_stats_cpu import SHAPES, check, make_input

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_float64_and_repeats_bitwise(cuda, shape):
    a = check(shape, cuda)
    b = ops.avgpool_bn_stats(make_input(shape, cuda), *shape[4:])
    for u, v in zip(a, b):  # two launches, the same bits: y, sum, sumsq
        assert torch.equal(u, v)


@pytest.mark.parametrize("case,message", [("C=12", "multiple of 8"), ("nchw", "channels-last"), ("fp32", "BFloat16"),
                                          ("window", "larger than the padded input")])
def test_argument_checks_raise(cuda, case, message):
    x = torch.randn(2, 12 if case == "C=12" else 16, 6, 6, device=cuda)
    x = x if case == "fp32" else x.bfloat16()
    x = x if case == "nchw" else x.contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match=message):
        ops.avgpool_bn_stats(x, 9 if case == "window" else 3, 2, 1)
