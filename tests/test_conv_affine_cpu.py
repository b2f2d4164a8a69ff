"""conv2d_bn_act's CPU implementation: the composition of the CPU conv2d_fwd and bn_apply, and an
eval-mode BatchNorm2d after F.conv2d to bf16 rounding."""
import pytest
import torch
import torch.nn.functional as F

import dedloc_amd.ops  # noqa: F401

OPS = torch.ops.dedloc
CL = torch.channels_last


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _case(N, Cin, H, Cout, k, stride, pad, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, H, generator=g).bfloat16().contiguous(memory_format=CL)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16().contiguous(memory_format=CL)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.normal_(generator=g)
        bn.running_mean.normal_(generator=g)
        bn.running_var.uniform_(0.5, 2.0, generator=g)
    P = (H + 2 * pad - k) // stride + 1
    res = torch.randn(N, Cout, P, P, generator=g).bfloat16().contiguous(memory_format=CL)
    return x, w, bn, res


@pytest.mark.parametrize("shape", [(2, 8, 9, 16, 3, 2, 1), (2, 3, 12, 8, 7, 2, 3), (3, 16, 5, 24, 1, 1, 0)])
@pytest.mark.parametrize("has_res,relu", [(False, False), (False, True), (True, False), (True, True)])
def test_cpu_op_is_the_composition_and_matches_eval_batchnorm(shape, has_res, relu):
    stride, pad = shape[5], shape[6]
    x, w, bn, res = _case(*shape)
    with torch.no_grad():
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        r = res if has_res else None
        y = OPS.conv2d_bn_act(x, w, scale, shift, r, relu, stride, pad)
        two = OPS.bn_apply(OPS.conv2d_fwd(x, w, stride, pad), r, scale, shift, torch.zeros_like(scale),
                           torch.ones_like(scale), relu, 1)
        assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
        assert torch.equal(y.view(torch.int16), two.view(torch.int16))
        ref = bn(F.conv2d(x.float(), w.float(), stride=stride, padding=pad))
        if has_res:
            ref = ref + res.float()
        if relu:
            ref = ref.relu()
    assert _rel(y, ref) < 1e-2


def test_cpu_op_rejects_bad_operands():
    x, w, bn, res = _case(2, 8, 9, 16, 3, 2, 1)
    scale, shift = torch.ones(16), torch.zeros(16)
    with pytest.raises((RuntimeError, AssertionError)):
        OPS.conv2d_bn_act(x, w, scale[:8], shift, None, False, 2, 1)
    with pytest.raises((RuntimeError, AssertionError)):
        OPS.conv2d_bn_act(x, w, scale.double(), shift, None, False, 2, 1)
    with pytest.raises((RuntimeError, AssertionError)):
        OPS.conv2d_bn_act(x, w, scale, shift, res[:, :, :-1], False, 2, 1)
