"""conv2d_bn_act on the GPU: the inference conv with a frozen BatchNorm's scale / shift, the residual
add and the ReLU in the epilogue (conv.hip's AFF instantiations; the GEMM route plus one bn_apply
pass for the wide stride-1 1x1 convs), at every route and tile shape conv2d_fwd takes."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dedloc_amd.ops  # noqa: F401

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc
CL = torch.channels_last

# (N, Cin, H, Cout, k, stride, pad)
SHAPES = [
    (2, 64, 14, 64, 3, 1, 1),       # 256x64 tile
    (2, 128, 14, 128, 3, 2, 1),     # 128x128 tile, stride 2
    (3, 512, 6, 512, 3, 2, 1),      # M = 27, far below a tile
    (2, 128, 9, 192, 3, 1, 1),      # Cout tail past one 128 tile
    (2, 256, 14, 128, 1, 1, 0),     # narrow 1x1 on conv.hip
    (2, 256, 14, 512, 1, 2, 0),     # strided 1x1
    (1, 1024, 7, 2048, 1, 2, 0),    # odd spatial size
    (2, 3, 32, 64, 7, 2, 3),        # stem, space-to-depth
    (2, 3, 31, 64, 7, 2, 3),        # stem, column fallback
    (8, 256, 32, 1024, 1, 1, 0),    # 128 gemm8 tiles: the GEMM route plus the bn_apply pass
]
VARIANTS = [(False, False), (False, True), (True, False), (True, True)]  # (res given, relu)


def _out_hw(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """Inputs whose every intermediate is exact in fp32 and whose output is exact in bf16, and the
    float64 conv of them (computed once per shape, shared by the four variants, never modified)."""
    N, Cin, H, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(hash(shape) & 0xFFFF)
    x = torch.randint(-4, 5, (N, Cin, H, H), generator=g).double()
    w = torch.zeros(Cout, Cin * k * k, dtype=torch.float64)
    taps = torch.stack([torch.randperm(Cin * k * k, generator=g)[:8] for _ in range(Cout)])
    w.scatter_(1, taps, (torch.randint(0, 2, (Cout, 8), generator=g) * 2 - 1).double())
    w = w.view(Cout, Cin, k, k)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=g)]
    shift = torch.randint(-8, 9, (Cout,), generator=g).float()
    P = _out_hw(H, k, stride, pad)
    res = torch.randint(-16, 17, (N, Cout, P, P), generator=g).double()
    c = F.conv2d(x, w, stride=stride, padding=pad)
    assert c.abs().max() <= 32
    return x, w, scale, shift, res, c


@functools.lru_cache(maxsize=None)
def _random_case(shape):
    N, Cin, H, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(1 + (hash(shape) & 0xFFFF))
    x = torch.randn(N, Cin, H, H, generator=g).bfloat16().contiguous(memory_format=CL)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16().contiguous(memory_format=CL)
    scale = torch.empty(Cout).uniform_(0.5, 1.5, generator=g)
    shift = torch.randn(Cout, generator=g)
    P = _out_hw(H, k, stride, pad)
    res = torch.randn(N, Cout, P, P, generator=g).bfloat16().contiguous(memory_format=CL)
    return x, w, scale, shift, res


def _bits(t):
    return t.contiguous(memory_format=CL).view(torch.int16)


def _ordered(t):
    """bf16 -> int32 keys in value order (adjacent representable values differ by 1; +0 and -0 agree)"""
    b = _bits(t).int()
    return torch.where(b >= 0, b, -(b & 0x7FFF))


@pytest.mark.parametrize("has_res,relu", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_inputs_match_float64_bitwise(cuda, shape, has_res, relu):
    N, Cin, H, Cout, k, stride, pad = shape
    x, w, scale, shift, res, c = _exact_case(shape)
    ref = c * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if has_res:
        ref = ref + res
    if relu:
        ref = ref.clamp_min(0)
    assert ref.abs().max() <= 88
    ref64, ref = ref, ref.to(torch.bfloat16)
    assert torch.equal(ref.double(), ref64)  # multiples of 1/2 below 128: exact in bf16
    y = OPS.conv2d_bn_act(x.bfloat16().to(cuda).contiguous(memory_format=CL),
                          w.bfloat16().to(cuda).contiguous(memory_format=CL), scale.to(cuda), shift.to(cuda),
                          res.bfloat16().to(cuda).contiguous(memory_format=CL) if has_res else None, relu, stride, pad)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
    assert torch.equal(_bits(y.cpu()), _bits(ref))


@pytest.mark.parametrize("has_res,relu", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_inputs_equal_the_two_kernel_form(cuda, shape, has_res, relu):
    N, Cin, H, Cout, k, stride, pad = shape
    x, w, scale, shift, res = (t.to(cuda) for t in _random_case(shape))
    r = res if has_res else None
    y = OPS.conv2d_bn_act(x, w, scale, shift, r, relu, stride, pad)
    c = OPS.conv2d_fwd(x, w, stride, pad)
    if Cout != 192:
        two = OPS.bn_apply(c, r, scale, shift, torch.zeros_like(scale), torch.ones_like(scale), relu, 1)
        assert torch.equal(_bits(y), _bits(two))
        return
    # bn_apply takes power-of-two channel counts only: the same expression in float64 arithmetic
    # rounded once to fp32 per step (mul, add, add) on conv2d_fwd's output.  A fused multiply-add and
    # mul-then-add round apart only within ~4 fp32 ulps of a bf16 rounding boundary, 2^-14 of the
    # values: at most 1 bf16 ulp on at most 1e-3 of the elements.
    bc = (1, -1, 1, 1)
    o = (c.double() * scale.double().view(bc)).float()
    o = (o.double() + shift.double().view(bc)).float()
    if has_res:
        o = (o.double() + r.double()).float()
    if relu:
        o = torch.where(o < 0, torch.zeros_like(o), o)
    d = (_ordered(y) - _ordered(o.to(torch.bfloat16))).abs()
    frac = (d > 0).float().mean().item()
    print(f"conv2d_bn_act Cout=192 res={has_res} relu={relu}: max ulp {int(d.max())}, differing {frac:.2e}")
    assert d.max() <= 1 and frac <= 1e-3


def test_domain_errors_raise(cuda):
    x, w, scale, shift, res = (t.to(cuda) for t in _random_case(SHAPES[0]))
    ok = OPS.conv2d_bn_act(x, w, scale, shift, res, True, 1, 1)
    assert ok.shape == res.shape
    with pytest.raises(RuntimeError, match="scale"):
        OPS.conv2d_bn_act(x, w, scale[:32].contiguous(), shift, None, True, 1, 1)
    with pytest.raises(RuntimeError, match="scale"):
        OPS.conv2d_bn_act(x, w, scale.bfloat16(), shift, None, True, 1, 1)
    with pytest.raises(RuntimeError, match="shift"):
        OPS.conv2d_bn_act(x, w, scale, shift.double(), None, True, 1, 1)
    with pytest.raises(RuntimeError, match="res"):
        OPS.conv2d_bn_act(x, w, scale, shift, res[:, :, :-1].contiguous(memory_format=CL), True, 1, 1)
    with pytest.raises(RuntimeError, match="res"):
        OPS.conv2d_bn_act(x, w, scale, shift, res[:1].contiguous(memory_format=CL), True, 1, 1)
    with pytest.raises(RuntimeError, match="channels-last"):
        OPS.conv2d_bn_act(x.contiguous(), w, scale, shift, None, True, 1, 1)
    torch.cuda.synchronize()
