"""Head_dim-64 attention kernels around their tile loops: the dQ kernel's lean -> masked loop
hand-over, its register bias-gradient tail, the paired 16-byte store epilogues of all three kernels
and the dK/dV kernel's strided staging, at the smallest shapes where each can go wrong.  A store
that lands right values in wrong columns shows up against the fp32 reference."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

D = 64


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ref(qkv, mask, H, S):
    T, ld = qkv.shape
    B = T // S
    x = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    bias = torch.where(mask.bool(), 0.0, float("-inf"))[:, None, None, :]
    o = F.scaled_dot_product_attention(x[0], x[1], x[2], attn_mask=bias)
    return o.permute(0, 2, 1, 3).reshape(B * S, H * D)


def _kvinfo(mask):
    lens = mask.sum(1).int()
    prefix = (mask.bool() == (torch.arange(mask.shape[1], device=mask.device) < lens[:, None])).all()
    return torch.cat([lens, prefix.int().view(1)]).contiguous()


def _check(cuda, S, lens, H=2, hole=False):
    import dedloc_amd.ops  # noqa: F401

    ops = torch.ops.dedloc
    torch.manual_seed(17)
    B, HD, scale = len(lens), H * D, 1 / math.sqrt(D)
    qkv = (torch.randn(B * S, 3 * HD, device=cuda) * 1.5).bfloat16()
    mask = (torch.arange(S, device=cuda)[None, :] < torch.tensor(lens, device=cuda)[:, None]).long()
    if hole:
        mask[0, 10:20] = 0  # not a prefix mask: every tile takes the additive-bias path
    mbias = torch.where(mask.bool(), 0.0, -1e30).float()
    kvinfo = _kvinfo(mask)
    assert kvinfo[-1].item() == (0 if hole else 1)
    out, lse = ops.attn_fwd(qkv, mbias, H, S, scale, kvinfo)
    qkv_r = qkv.float().requires_grad_(True)
    ref = _ref(qkv_r, mask, H, S)
    e = rel(out, ref)
    print("O", e)
    assert e < 1.5e-2, e
    dout = torch.randn_like(out)
    dbias = torch.full((3 * HD,), 0.25, device=cuda)
    dqkv = ops.attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo, dbias)
    g_ref = torch.autograd.grad(ref, qkv_r, dout.float())[0]
    for part in range(3):
        sl = slice(part * HD, (part + 1) * HD)
        e = rel(dqkv[:, sl], g_ref[:, sl])
        print("dQ dK dV".split()[part], e)
        assert e < 3e-2, (part, e)
    eq = rel(dbias[:HD] - 0.25, dqkv[:, :HD].float().sum(0))
    ev = rel(dbias[2 * HD:] - 0.25, dout.float().sum(0))
    print("dbias q", eq, "v", ev)
    assert eq < 1e-4, eq
    assert ev < 1e-4, ev
    assert torch.equal(dbias[HD:2 * HD], torch.full_like(dbias[HD:2 * HD], 0.25))  # key bias: untouched
    again = ops.attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo, torch.zeros_like(dbias))
    assert torch.equal(dqkv, again)


def test_one_boundary_tile_dead_waves(cuda):
    """S = 64: nlean is 1 or 0, and three of the four waves of the 256-query block hold no row."""
    _check(cuda, 64, (64, 33, 1))


def test_lean_to_boundary_handover_odd_nlean(cuda):
    """S = 128: lean only (128), one lean tile then the boundary tile (65: ring slot parity), and a
    second key block that is all padding (64: the dK/dV early exit)."""
    _check(cuda, 128, (128, 65, 64))


def test_two_query_blocks_odd_tile_count(cuda):
    """S = 320: five tiles, the second 256-query block holds 64 live rows."""
    _check(cuda, 320, (320, 257))


def test_non_prefix_mask_all_tiles_masked(cuda):
    """A hole in the mask: nlean = 0, the bias reaches the masked loop through the ring stage."""
    _check(cuda, 128, (128, 128), hole=True)


def test_odd_head_count_block_remap(cuda):
    """S = 192, H = 3, 8 sequences: block counts are multiples of 8, so the XCD block remap is
    active with an odd head count, and the last query block is partly empty."""
    _check(cuda, 192, (192, 192, 100, 64, 1, 129, 191, 192), H=3)
