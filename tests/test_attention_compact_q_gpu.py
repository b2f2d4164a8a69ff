"""The head_dim-64 attention kernels with compact queries (``ops.attn_fwd_q`` / ``attn_bwd_q``,
docs/KERNELS.md "Compact queries") against the same kernels on the full buffer.

Layout under test: sequence b's queries are the first qcnt[b] rows of its slot of Sq rows in
q [B*Sq, H*64]; keys and values stay in the fused [B*S, 3*H*64] QKV buffer (passed as its K | V
column slice).  B = 3, H = 2; S in {128, 192}, Sq in {64, 128}; live counts 1 ([CLS] only), 31, 33,
64, 65 and Sq: across the 32-row sub-block, the 64-row tile and the slot's end; rows drawn in
random order with row 0 ([CLS]) first; key masks: none, a right-padded one whose boundary falls
inside a tile (kvinfo lengths), and a generic additive one (a hole: every tile takes the bias path).

Rows are placed in two ways.  "kept": a row sits in the half (rows 0-31 or 32-63) of a 64-row tile
that it occupies in its own sequence, as models/albert.py places them.  "random": any row anywhere,
row 0 first.

Forward:  out and lse of every live compact row equal the same rows of ``attn_fwd`` on the full
          buffer bit for bit (the key-tile order per query is the same) for every "kept" case and
          for the generic mask; dead rows of out are zero.  NOT bit-equal, measured on an MI355X:
          "random" placement under no mask or a length mask, i.e. whenever a row that runs through
          the lean tile loop changes its 32-row sub-block within the wave (19-38 % of the out
          elements one bf16 step apart, 7-12 % of the lse one fp32 step; rows that change place but
          keep their sub-block: none).  Cause: the lean loop's row maximum (vmax3, inline asm) reads
          the score accumulators right behind the MFMA chain, and which stale value it can see
          depends on the sub-block's place in the instruction stream; the maximum is only the
          deferred-rescale reference point, so both results are equally near the fp32 reference
          (tests/test_attention_varlen_gpu.py describes the same effect at head_dim 128).  Those
          cases are held to the bounds of the existing attention tests against the fp32 reference
          (out 1.5e-2, lse 1e-2, gradients 3e-2, norm-wise) and to the full path's own error on the
          same rows: the two are the same arithmetic from two reference points, that is two
          independent sets of bf16 roundings over at least 65 rows x 128 columns, so their errors
          agree to a few percent, while a wrong row, column or tile moves the error to order 1;
          the compact error may be at most 1.5 times the full path's (lse: plus 1e-6, a few fp32
          steps, since its own error is of that size).
Backward: against ``attn_bwd`` on the full buffer with dout zero outside the chosen rows.  Where
          the forward is bit-equal, dQ rows are bit-equal too (dead rows zero).  delta is not an
          output of the full op, so it is checked bit for bit, in every case, against the kernels'
          own summation replayed in fp32 (bf16 products are exact in fp32, so the fused
          multiply-adds of the kernel are plain adds of exact products: 32 sequential adds per
          half-row, then the two halves).  dK / dV change their summation order over queries and
          are not bit-equal: they, and the bias gradients, are held to the bounds of
          tests/test_attention_tails_gpu.py against the fp32 reference (3e-2 norm-wise per third;
          bias gradient 1e-4 against the column sums of what was stored; key third of the bias
          gradient untouched).  Where the forward is bit-equal the compact path's error may not
          exceed the full path's by more than 2.2e-4: both sum the same non-zero bf16 products in
          fp32 (the rows the full path adds on top carry exact zeros), so they differ by fp32
          reassociation, about n * 2^-24 relative for n <= 192 terms; that flips the bf16 rounding
          of a share of about n * 2^-16 of the elements by one step of 2^-8 relative, which moves
          the norm-wise error by at most sqrt(192 * 2^-16) * 2^-8 = 2.1e-4.  Elsewhere: the factor
          1.5 above.
Identity: with every row selected in its own order the compact result equals the full one, dK / dV
          included (same query-tile order).

Every case prints its figures as one JSON line before it asserts."""
import functools
import json
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, H, D = 3, 2, 64
HD = H * D
SCALE = 1.0 / math.sqrt(D)
COUNTS = {64: ((1, 31, 33), (64, 33, 1)), 128: ((1, 31, 33), (64, 65, 128))}
MASKS = ("none", "padded", "generic")
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
    print(json.dumps({"case": case, **{k: (round(v, 8) if isinstance(v, float) else v) for k, v in figures.items()}}))


@functools.lru_cache(maxsize=None)
def _full(S, mask_kind):
    """One full problem per (S, mask), shared by its cases and left unchanged: inputs, the key mask
    in both forms, and the full kernels' forward."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5 + S + len(mask_kind))
    qkv = (torch.randn(B * S, 3 * HD, device=dev, generator=g) * 1.5).bfloat16()
    lens = {"none": (S, S, S), "padded": (S, S - 27, 70), "generic": (S, S, S - 27)}[mask_kind]
    mask = torch.arange(S, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]
    if mask_kind == "generic":
        mask[0, 10:20] = False
    klen = mask.sum(1).int()
    prefix = (mask == (torch.arange(S, device=dev) < klen[:, None])).all()
    kvinfo = torch.cat([klen, prefix.int().view(1)]).contiguous()
    assert kvinfo[-1].item() == (0 if mask_kind == "generic" else 1)
    mbias = torch.where(mask, 0.0, -1e30).float().contiguous()
    out, lse = OPS.attn_fwd(qkv, mbias, H, S, SCALE, kvinfo)
    x = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    sc = torch.matmul(x[0], x[1].transpose(-1, -2)) * SCALE + torch.where(mask, 0.0, float("-inf"))[:, None, None, :]
    ref_lse = (torch.logsumexp(sc, -1) * math.log2(math.e)).permute(0, 2, 1).reshape(B * S, H)
    ref_out = torch.matmul(torch.softmax(sc, -1), x[2]).permute(0, 2, 1, 3).reshape(B * S, HD)
    return dict(qkv=qkv, mask=mask, mbias=mbias, kvinfo=kvinfo, out=out, lse=lse, ref_out=ref_out, ref_lse=ref_lse)


def _ref_grad(qkv, mask, S, dout):
    """fp32 reference gradient of the full problem: [B*S, 3*H*D]."""
    qkv_r = qkv.float().requires_grad_(True)
    x = qkv_r.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    bias = torch.where(mask, 0.0, float("-inf"))[:, None, None, :]
    o = F.scaled_dot_product_attention(x[0], x[1], x[2], attn_mask=bias).permute(0, 2, 1, 3).reshape(B * S, HD)
    return torch.autograd.grad(o, qkv_r, dout.float())[0]


def _plan(S, Sq, counts, place="random"):
    """rows [B, Sq] (positions inside each sequence: row 0 first, then a random draw, for "kept"
    from the rows of the place's own half of a 64-row tile; the padding repeats row 0), the flat
    compact -> full row map, and the live mask [B*Sq]."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(S + Sq + sum(counts))
    rows = torch.zeros(B, Sq, dtype=torch.long)
    for b, n in enumerate(counts):
        if place == "identity":
            rows[b, 1:n] = torch.arange(1, n)
        elif place == "random":
            rows[b, 1:n] = torch.randperm(S - 1, generator=g)[:n - 1] + 1
        else:
            perm = torch.randperm(S - 1, generator=g) + 1
            pools = [perm[(perm // 32) % 2 == h].tolist() for h in (0, 1)]
            for p in range(1, n):
                rows[b, p] = pools[(p // 32) % 2].pop()
    live = torch.arange(Sq)[None, :] < torch.tensor(counts)[:, None]
    full_rows = (torch.arange(B)[:, None] * S + rows).reshape(-1)
    return full_rows.to(dev), live.reshape(-1).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev)


def _delta_replay(dout, out):
    """rowsum(dO * O) per head in the dQ kernel's order: a lane holds columns 16 ks + 8 hh + e of
    its row (ks 0..3, e 0..7) and adds them one by one; the two half-rows (hh) are added last."""
    p = dout.float().reshape(-1, H, 4, 2, 8) * out.float().reshape(-1, H, 4, 2, 8)  # row, head, ks, hh, e
    acc = torch.zeros(p.shape[0], H, 2, device=p.device)
    for ks in range(4):
        for e in range(8):
            acc = acc + p[:, :, ks, :, e]
    return acc[:, :, 0] + acc[:, :, 1]  # [rows, H]


def _run_case(S, Sq, counts, mask_kind, place="random"):
    f = _full(S, mask_kind)
    dev = f["qkv"].device
    full_rows, live, qcnt = _plan(S, Sq, counts, place)
    q = f["qkv"][:, :HD].index_select(0, full_rows).contiguous()
    kv = f["qkv"][:, HD:]  # K | V where they are, in the fused buffer
    out_c, lse_c = OPS.attn_fwd_q(q, kv, qcnt, f["mbias"], H, S, SCALE, f["kvinfo"])
    lr, cr = full_rows[live], torch.nonzero(live).squeeze(1)  # full rows of the live compact rows

    # ---- forward: bit-equal live rows, zero dead rows
    lse_full = f["lse"].permute(0, 2, 1).reshape(B * S, H)
    lse_comp = lse_c.permute(0, 2, 1).reshape(B * Sq, H)
    fwd = dict(out_equal=torch.equal(out_c[cr], f["out"][lr]), lse_equal=torch.equal(lse_comp[cr], lse_full[lr]),
               dead_out_zero=bool((out_c[~live] == 0).all()),
               out_c=rel(out_c[cr], f["ref_out"][lr]), out_f=rel(f["out"][lr], f["ref_out"][lr]),
               lse_c=rel(lse_comp[cr], f["ref_lse"][lr]), lse_f=rel(lse_full[lr], f["ref_lse"][lr]))

    # ---- backward inputs: random dout on every compact row (dead rows must be ignored), the full
    # problem gets the live ones at their rows and zero elsewhere
    g = torch.Generator(device=dev).manual_seed(3)
    dout_c = torch.randn(B * Sq, HD, device=dev, generator=g).bfloat16()
    dout_f = torch.zeros(B * S, HD, device=dev, dtype=torch.bfloat16)
    dout_f[lr] = dout_c[cr]
    db_f = torch.full((3 * HD,), 0.25, device=dev)
    db_c = torch.full((3 * HD,), 0.25, device=dev)
    dqkv_f = OPS.attn_bwd(f["qkv"], f["mbias"], f["out"], dout_f, f["lse"], H, S, SCALE, f["kvinfo"], db_f)
    dq_c, dkv_c, delta_c = OPS.attn_bwd_q(q, kv, qcnt, f["mbias"], out_c, dout_c, lse_c, H, S, SCALE, f["kvinfo"], db_c)
    g_ref = _ref_grad(f["qkv"], f["mask"], S, dout_f)
    delta_comp = delta_c.permute(0, 2, 1).reshape(B * Sq, H)
    bwd = dict(dq_equal=torch.equal(dq_c[cr], dqkv_f[lr, :HD]), dead_dq_zero=bool((dq_c[~live] == 0).all()),
               delta_equal=torch.equal(delta_comp[cr], _delta_replay(dout_c[cr], out_c[cr])),
               dk_c=rel(dkv_c[:, :HD], g_ref[:, HD:2 * HD]), dk_f=rel(dqkv_f[:, HD:2 * HD], g_ref[:, HD:2 * HD]),
               dv_c=rel(dkv_c[:, HD:], g_ref[:, 2 * HD:]), dv_f=rel(dqkv_f[:, 2 * HD:], g_ref[:, 2 * HD:]),
               dq_c=rel(dq_c[cr], g_ref[lr, :HD]), dq_f=rel(dqkv_f[lr, :HD], g_ref[lr, :HD]),
               dbq_c=rel(db_c[:HD] - 0.25, dq_c[cr].float().sum(0)), dbq_f=rel(db_f[:HD] - 0.25, dqkv_f[:, :HD].float().sum(0)),
               dbv_c=rel(db_c[2 * HD:] - 0.25, dout_c[cr].float().sum(0)), dbv_f=rel(db_f[2 * HD:] - 0.25, dout_f.float().sum(0)),
               dbk_untouched=torch.equal(db_c[HD:2 * HD], torch.full_like(db_c[HD:2 * HD], 0.25)),
               dkv_equal=torch.equal(dkv_c, dqkv_f[:, HD:]), finite=bool(torch.isfinite(dkv_c.float()).all()))
    return fwd, bwd


CASES = [(S, Sq, c, m, p) for S in (128, 192) for Sq in (64, 128) for c in COUNTS[Sq] for m in MASKS
         for p in ("kept", "random")]


@pytest.mark.parametrize("S,Sq,counts,mask_kind,place", CASES,
                         ids=[f"S{S}-Sq{Sq}-{'_'.join(map(str, c))}-{m}-{p}" for S, Sq, c, m, p in CASES])
def test_compact_rows_against_full_buffer(S, Sq, counts, mask_kind, place):
    fwd, bwd = _run_case(S, Sq, counts, mask_kind, place)
    _record(f"S{S} Sq{Sq} {counts} {mask_kind} {place}", **fwd, **bwd)
    exact = place == "kept" or mask_kind == "generic"  # see the module docstring
    assert fwd["dead_out_zero"] and bwd["dead_dq_zero"] and bwd["delta_equal"] and bwd["finite"], (fwd, bwd)
    assert fwd["out_f"] < 1.5e-2 and fwd["out_c"] < 1.5e-2 and fwd["lse_f"] < 1e-2 and fwd["lse_c"] < 1e-2, fwd
    if exact:
        assert fwd["out_equal"] and fwd["lse_equal"], fwd
        assert bwd["dq_equal"], bwd
    else:
        assert fwd["out_c"] <= 1.5 * fwd["out_f"] and fwd["lse_c"] <= 1.5 * fwd["lse_f"] + 1e-6, fwd
        assert bwd["dq_c"] <= 1.5 * bwd["dq_f"], bwd
    for part in ("dq", "dk", "dv"):
        assert bwd[part + "_f"] < 3e-2 and bwd[part + "_c"] < 3e-2, (part, bwd)
    for part in ("dk", "dv"):
        if exact:
            assert bwd[part + "_c"] <= bwd[part + "_f"] + 2.2e-4, (part, bwd)
        else:
            assert bwd[part + "_c"] <= 1.5 * bwd[part + "_f"], (part, bwd)
    for part in ("dbq", "dbv"):
        assert bwd[part + "_f"] < 1e-4 and bwd[part + "_c"] < 1e-4, (part, bwd)
    assert bwd["dbk_untouched"], bwd


@pytest.mark.parametrize("mask_kind", MASKS)
def test_every_row_selected_equals_full_path(mask_kind):
    S = 128
    fwd, bwd = _run_case(S, S, (S, S, S), mask_kind, "identity")
    _record(f"identity S{S} {mask_kind}", **fwd, **bwd)
    assert fwd["out_equal"] and fwd["lse_equal"], fwd
    assert bwd["dq_equal"] and bwd["delta_equal"] and bwd["dkv_equal"], bwd
    assert bwd["dbq_c"] < 1e-4 and bwd["dbv_c"] < 1e-4 and bwd["dbk_untouched"], bwd


def test_repeatable_and_contract(cuda):
    """Two runs give the same bits; layouts the kernels do not serve are refused, not computed."""
    S, Sq = 128, 64
    f = _full(S, "padded")
    full_rows, live, qcnt = _plan(S, Sq, (64, 33, 1))
    q = f["qkv"][:, :HD].index_select(0, full_rows).contiguous()
    kv = f["qkv"][:, HD:]
    a = OPS.attn_fwd_q(q, kv, qcnt, f["mbias"], H, S, SCALE, f["kvinfo"])
    b = OPS.attn_fwd_q(q, kv, qcnt, f["mbias"], H, S, SCALE, f["kvinfo"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][:, :, :1], b[1][:, :, :1])
    with pytest.raises(RuntimeError, match="multiple of 64"):  # a slot of 32 rows
        OPS.attn_fwd_q(q[:B * 32], kv, qcnt, f["mbias"], H, S, SCALE, f["kvinfo"])
    with pytest.raises(RuntimeError, match="head_dim 64"):  # one head of 128
        OPS.attn_fwd_q(q, kv, qcnt, f["mbias"], 1, S, SCALE, f["kvinfo"])
    with pytest.raises(RuntimeError, match="qcnt"):
        OPS.attn_fwd_q(q, kv, qcnt[:2], f["mbias"], H, S, SCALE, f["kvinfo"])
