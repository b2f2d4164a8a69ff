"""The fused flash-attention kernels at head_dim 128 (attention_hd128.hip), called directly through
``torch.ops.dedloc.attn_fwd`` / ``attn_bwd``, against an fp32 PyTorch reference
(scaled_dot_product_attention + autograd): outputs, log2-unit lse, packed dQKV, the fused QKV bias
gradient, both mask forms, the rescale paths, the composed path on the same inputs, repeatability
and one model-level comparison.  The bounds are the ones the head_dim-64 kernels are held to in
test_kernels_gpu.py / test_attention_composed.py.

Every case prints the errors it measured as one JSON line (and appends it to the file named by
ATTN_HD128_MARGINS, if set): profiles/attn_hd128_margins.jsonl is such a run.

Grids: forward, dQ and dK/dV all launch (S / 128 rounded up) x H x B workgroups, so the XCD block
renumbering (on when the workgroup count is a multiple of 8) is on or off for all three together."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)
OPS = None


@pytest.fixture(autouse=True)
def _ops(cuda):
    global OPS
    import dedloc_amd.ops  # noqa: F401

    OPS = torch.ops.dedloc


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _record(case, **figures):
    line = json.dumps({"case": case, **{k: (round(v, 8) if isinstance(v, float) else v) for k, v in figures.items()}})
    print(line)
    path = os.environ.get("ATTN_HD128_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _attn_ref(qkv, mask, H, S, dout=None):
    """fp32 reference: out [B*S, H*D], lse [B, H, S] in log2 units, and (with dout) dQKV packed."""
    T, ld = qkv.shape
    B = T // S
    qkv_r = qkv.float().detach().requires_grad_(True)
    x = qkv_r.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    bias = torch.where(mask.bool(), 0.0, float("-inf"))[:, None, None, :]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias)
    o = o.permute(0, 2, 1, 3).reshape(B * S, H * D)
    with torch.no_grad():
        lse = torch.logsumexp(torch.matmul(q, k.transpose(-1, -2)) * SCALE + bias, -1) * math.log2(math.e)
    g = torch.autograd.grad(o, qkv_r, dout.float())[0] if dout is not None else None
    return o.detach(), lse, g


def _kvinfo(mask):
    lens = mask.sum(1).int()
    prefix = (mask.bool() == (torch.arange(mask.shape[1], device=mask.device) < lens[:, None])).all()
    return torch.cat([lens, prefix.int().view(1)]).contiguous()


def _mbias(mask):
    return torch.where(mask.bool(), 0.0, -1e30).float()


def _check_grads(case, dqkv, g_ref, H, figures):
    for part, name in enumerate(("dq", "dk", "dv")):
        sl = slice(part * H * D, (part + 1) * H * D)
        figures[name] = rel(dqkv[:, sl], g_ref[:, sl])
    _record(case, **figures)
    for name in ("dq", "dk", "dv"):
        assert figures[name] < 3e-2, (name, figures[name])


# workgroups per grid = ceil(S / 128) * H * B:
#   (2, 2, 64) -> 4: remap off, one key tile (the ring is never refilled)
#   (2, 4, 128) -> 8: remap ON, one wrap of the two-slot ring
#   (1, 3, 192) -> 6: remap off, last query / key block half empty, ld = 3*3*128 (no power of two)
#   (3, 1, 320) -> 9: remap off, three blocks, the last one half empty, H = 1
#   (1, 2, 512) -> 8: remap ON, four full blocks
@pytest.mark.parametrize("B,H,S", [(2, 2, 64), (2, 4, 128), (1, 3, 192), (3, 1, 320), (1, 2, 512)])
def test_shapes(cuda, B, H, S):
    torch.manual_seed(1)
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    mask = torch.ones(B, S, device=cuda, dtype=torch.long)
    mask[-1, S - S // 4:] = 0  # through mbias only (no kvinfo)
    mbias = _mbias(mask)
    out, lse = OPS.attn_fwd(qkv, mbias, H, S, SCALE, None)
    dout = torch.randn_like(out)
    dbias = torch.full((3 * H * D,), 0.25, device=cuda)  # pre-filled: the kernel accumulates
    dqkv = OPS.attn_bwd(qkv, mbias, out, dout, lse, H, S, SCALE, None, dbias)
    ref, lse_ref, g_ref = _attn_ref(qkv, mask, H, S, dout)
    HD = H * D
    bref = g_ref.sum(0)
    fig = {
        "out": rel(out, ref),
        "lse": (lse - lse_ref).abs().max().item(),
        "dbias_q_vs_colsum": rel(dbias[:HD] - 0.25, dqkv[:, :HD].float().sum(0)),
        "dbias_q_vs_ref": rel(dbias[:HD] - 0.25, bref[:HD]),
        "dbias_v_vs_colsum": rel(dbias[2 * HD:] - 0.25, dout.float().sum(0)),
    }
    assert out.shape == (B * S, HD) and lse.shape == (B, H, S) and dqkv.shape == qkv.shape
    _check_grads(f"shapes B={B} H={H} S={S}", dqkv, g_ref, H, fig)
    assert fig["out"] < 1.5e-2, fig
    assert fig["lse"] < 1e-2, fig
    assert fig["dbias_q_vs_colsum"] < 1e-4, fig
    assert fig["dbias_q_vs_ref"] < 3e-2, fig
    assert torch.equal(dbias[HD:2 * HD], torch.full_like(dbias[HD:2 * HD], 0.25))  # key part untouched
    assert fig["dbias_v_vs_colsum"] < 1e-4, fig


@pytest.mark.parametrize("lens", [(256, 200, 64, 37), (256, 256, 256, 256), (1, 65, 128, 255)])
def test_kv_lengths(cuda, lens):
    """Right-padded masks via kvinfo: padded key tiles are skipped, the boundary tile is masked,
    keys past a row's length get exactly zero dK / dV."""
    torch.manual_seed(3)
    B, H, S = len(lens), 2, 256
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    mask = (torch.arange(S, device=cuda)[None, :] < torch.tensor(lens, device=cuda)[:, None]).long()
    mbias = _mbias(mask)
    kvinfo = _kvinfo(mask)
    assert kvinfo[-1].item() == 1
    out, lse = OPS.attn_fwd(qkv, mbias, H, S, SCALE, kvinfo)
    out_b, _ = OPS.attn_fwd(qkv, mbias, H, S, SCALE, None)  # generic bias path
    dout = torch.randn_like(out)
    dqkv = OPS.attn_bwd(qkv, mbias, out, dout, lse, H, S, SCALE, kvinfo, None)
    ref, lse_ref, g_ref = _attn_ref(qkv, mask, H, S, dout)
    fig = {"out": rel(out, ref), "lse": (lse - lse_ref).abs().max().item(), "out_vs_generic": rel(out, out_b)}
    _check_grads(f"kv_lengths {lens}", dqkv, g_ref, H, fig)
    assert fig["out"] < 1.5e-2, fig
    assert fig["lse"] < 1e-2, fig
    assert fig["out_vs_generic"] < 1e-2, fig
    for b, n in enumerate(lens):
        if n < S:
            assert dqkv[b * S + n:(b + 1) * S, H * D:].abs().max().item() == 0.0


def test_non_prefix_mask_with_kvinfo(cuda):
    """kvinfo present but its prefix flag is 0 (a hole in the mask): the generic bias path, forward
    and backward."""
    torch.manual_seed(4)
    B, H, S = 2, 2, 128
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    mask = torch.ones(B, S, device=cuda, dtype=torch.long)
    mask[0, 10:20] = 0
    mbias = _mbias(mask)
    kvinfo = _kvinfo(mask)
    assert kvinfo[-1].item() == 0
    out, lse = OPS.attn_fwd(qkv, mbias, H, S, SCALE, kvinfo)
    dout = torch.randn_like(out)
    dqkv = OPS.attn_bwd(qkv, mbias, out, dout, lse, H, S, SCALE, kvinfo, None)
    ref, lse_ref, g_ref = _attn_ref(qkv, mask, H, S, dout)
    fig = {"out": rel(out, ref), "lse": (lse - lse_ref).abs().max().item()}
    _check_grads("non_prefix_mask", dqkv, g_ref, H, fig)
    assert fig["out"] < 1.5e-2, fig
    assert fig["lse"] < 1e-2, fig
    # the masked keys of row 0 get no gradient
    assert dqkv[10:20, H * D:].abs().max().item() == 0.0


def _fwd_bwd_unmasked(case, cuda, qkv, B, H, S):
    out, lse = OPS.attn_fwd(qkv, None, H, S, SCALE, None)
    dout = torch.randn_like(out)
    dqkv = OPS.attn_bwd(qkv, None, out, dout, lse, H, S, SCALE, None, None)
    ref, lse_ref, g_ref = _attn_ref(qkv, torch.ones(B, S, device=cuda), H, S, dout)
    fig = {"out": rel(out, ref), "lse": (lse - lse_ref).abs().max().item()}
    _check_grads(case, dqkv, g_ref, H, fig)
    assert fig["out"] < 1.5e-2, fig
    assert fig["lse"] < 1e-2, fig


def test_rescale_late_spike(cuda):
    """Forces the online-softmax rescale: one key spikes (x12) late in the sequence."""
    torch.manual_seed(6)
    B, H, S = 1, 2, 256
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    qkv[200, H * D:2 * H * D] *= 12
    _fwd_bwd_unmasked("rescale_late_spike", cuda, qkv, B, H, S)


def test_rescale_ramp(cuda):
    """Deferred-max rescale: key magnitudes ramp up tile by tile, at a different rate per head, so
    rows cross the rescale threshold at different tiles and some never do."""
    torch.manual_seed(5)
    B, H, S = 2, 4, 512
    qkv = torch.randn(B * S, 3 * H * D, device=cuda) * 1.5
    ramp = 1.0 + torch.arange(S, device=cuda).float() / 64.0  # grows per 64-key tile
    for h in range(H):
        cols = slice(H * D + h * D, H * D + (h + 1) * D)
        qkv[:, cols] *= (ramp.repeat(B) ** (0.5 * h))[:, None]
    _fwd_bwd_unmasked("rescale_ramp", cuda, qkv.bfloat16(), B, H, S)


def test_matches_composed_path(cuda):
    """The fused kernels and the composed path (GEMMs + softmax kernel) on the same inputs."""
    import dedloc_amd.ops as ops

    torch.manual_seed(0)
    B, H, S = 2, 2, 128
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    mask = torch.ones(B, S, device=cuda, dtype=torch.long)
    mask[-1, S - S // 4:] = 0
    mbias = _mbias(mask)
    dout = torch.randn(B * S, H * D, device=cuda).bfloat16()
    out_c, lse_c = ops.attn_composed_fwd(qkv, mbias, H, S, SCALE)
    db_c = torch.zeros(3 * H * D, device=cuda)
    g_c = ops.attn_composed_bwd(qkv, mbias, out_c, dout, lse_c, H, S, SCALE, db_c)
    out_f, lse_f = OPS.attn_fwd(qkv, mbias, H, S, SCALE, None)
    db_f = torch.zeros_like(db_c)
    g_f = OPS.attn_bwd(qkv, mbias, out_f, dout, lse_f, H, S, SCALE, None, db_f)
    fig = {"out": rel(out_c, out_f), "lse": (lse_c - lse_f).abs().max().item(), "dqkv": rel(g_c, g_f),
           "dbias": rel(db_c, db_f)}
    _record("matches_composed", **fig)
    assert fig["out"] < 1e-2, fig
    assert fig["lse"] < 1e-3, fig
    assert fig["dqkv"] < 2e-2, fig
    assert fig["dbias"] < 2e-2, fig


def test_repeatable(cuda):
    """Two calls on the same input are bit-equal: the forward, and the backward's dQKV (dQ, dK and
    dV are written by plain stores, one writer per element; only dbias is accumulated with
    atomics, so it is left out here)."""
    torch.manual_seed(7)
    B, H, S = 3, 2, 320
    qkv = (torch.randn(B * S, 3 * H * D, device=cuda) * 1.5).bfloat16()
    mask = (torch.arange(S, device=cuda)[None, :] < torch.tensor((320, 130, 64), device=cuda)[:, None]).long()
    mbias, kvinfo = _mbias(mask), _kvinfo(mask)
    out1, lse1 = OPS.attn_fwd(qkv, mbias, H, S, SCALE, kvinfo)
    out2, lse2 = OPS.attn_fwd(qkv, mbias, H, S, SCALE, kvinfo)
    assert torch.equal(out1, out2) and torch.equal(lse1, lse2)
    dout = torch.randn_like(out1)
    g1 = OPS.attn_bwd(qkv, mbias, out1, dout, lse1, H, S, SCALE, kvinfo, None)
    g2 = OPS.attn_bwd(qkv, mbias, out1, dout, lse1, H, S, SCALE, kvinfo, None)
    assert torch.equal(g1, g2)


def test_model_fused_matches_composed(cuda):
    """A small ALBERT with two 128-wide heads, one batch of the synthetic stream with the mask it
    comes with: the fused attention path against the composed one (FUSED_HEAD_DIMS narrowed to 64),
    loss and flat gradient."""
    import dedloc_amd.ops as ops
    from dedloc_amd.data.synthetic_mlm import SyntheticSOPStream
    from dedloc_amd.models.albert import AlbertConfig, AlbertForPreTraining

    torch.manual_seed(0)
    cfg = AlbertConfig.tiny(hidden_size=256, num_attention_heads=2, intermediate_size=1024)
    model = AlbertForPreTraining(cfg)
    model.materialize(cuda)
    model.eval()
    batch = SyntheticSOPStream(4, 128, cfg.vocab_size, seed=0, device=cuda).next_batch()

    def step():
        out = model(batch["input_ids"], batch["attention_mask"], batch["token_type_ids"],
                    sentence_order_label=batch["sentence_order_label"], mlm_positions=batch["mlm_positions"],
                    mlm_labels=batch["mlm_labels"])
        out["loss"].backward()
        g = model.flat.grad.detach().clone()
        model.flat.grad.zero_()
        return float(out["loss"].detach()), g

    saved = ops.FUSED_HEAD_DIMS
    try:
        ops.FUSED_HEAD_DIMS = (64, 128)
        loss_f, g_f = step()
        ops.FUSED_HEAD_DIMS = (64,)
        loss_c, g_c = step()
    finally:
        ops.FUSED_HEAD_DIMS = saved
    fig = {"loss_fused": loss_f, "loss_composed": loss_c, "grad": rel(g_f, g_c)}
    _record("model_fused_vs_composed", **fig)
    assert math.isfinite(loss_f) and torch.isfinite(g_f).all()
    assert abs(loss_f - loss_c) < 2e-2, fig
    assert fig["grad"] < 5e-2, fig


def test_unsupported_head_dim_raises(cuda):
    """A head size that is neither 64 nor 128 is an error that names the supported sizes."""
    H, S, d = 2, 64, 32
    qkv = torch.randn(S, 3 * H * d, device=cuda).bfloat16()
    with pytest.raises(RuntimeError) as e:
        OPS.attn_fwd(qkv, None, H, S, 1.0 / math.sqrt(d), None)
    assert "supported head sizes are 64 and 128" in str(e.value), str(e.value)
    out = torch.zeros(S, H * d, device=cuda).bfloat16()
    lse = torch.zeros(1, H, S, device=cuda)
    with pytest.raises(RuntimeError) as e:
        OPS.attn_bwd(qkv, None, out, out, lse, H, S, 1.0 / math.sqrt(d), None, None)
    assert "supported head sizes are 64 and 128" in str(e.value), str(e.value)
