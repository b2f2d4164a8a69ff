"""Compact queries over a packed batch (``ops.attn_varlen_fwd_q`` / ``attn_varlen_bwd_q``) against the
packed kernels on the full buffer and the fp32 CPU op.  One buffer, H = 2, key lengths LENS: slots of
320 (lean tiles and a boundary tile), 128 (a slot less one key), 64 (exactly a slot), 64, 128, and a
dummy tail of 64 without queries; Sq = 128 exceeds the 64-row slots.  "kept" rows sit in the half of a
64-row tile that they have in their own sequence (models/albert.py), "random" ones anywhere.  Bounds
and reasons: tests/test_attention_compact_q_gpu.py (bit-equal where "kept"; else, and for dK | dV and
the bias gradient, 1.5 x the full path's norm-wise error against fp32; delta replayed in fp32)."""
import functools

import pytest
import torch

import dedloc_amd.ops  # noqa: F401  (registers torch.ops.dedloc)
from dedloc_amd.data.packing import make_seqinfo
from test_attention_compact_q_gpu import H, HD, SCALE, _delta_replay, rel  # 2 heads of 64; the same helpers

pytestmark = pytest.mark.gpu

LENS = (300, 127, 64, 40, 100, 64)
CASES = [(64, (64, 33, 31, 1, 0, 0)), (128, (128, 65, 64, 33, 1, 0)), (128, (1, 65, 0, 31, 64, 0))]


@functools.lru_cache(maxsize=None)
def _full():
    """The packed problem, shared by the cases and left unchanged: inputs, layout, the full forward."""
    dev = torch.device("cuda")
    seqinfo, host, rows, _ = make_seqinfo(LENS, dev, tail=False)
    g = torch.Generator(device=dev).manual_seed(11)
    qkv = (torch.randn(rows[-1], 3 * HD, device=dev, generator=g) * 1.5).bfloat16()
    out, lse = torch.ops.dedloc.attn_varlen_fwd(qkv, seqinfo, host, H, SCALE)
    return dict(qkv=qkv, seqinfo=seqinfo, host=host, rows=rows, out=out, lse=lse)


def _plan(rows, Sq, counts, place):
    """(compact place -> row of the packed buffer, the padding repeating row 0; live mask [n*Sq]; q; kv; qcnt)"""
    g = torch.Generator().manual_seed(Sq + sum(counts))
    full_rows = torch.tensor(rows[:-1])[:, None].repeat(1, Sq)
    for b, n in enumerate(counts):
        perm = torch.randperm(LENS[b] - 1, generator=g) + 1
        pools = [perm[(perm // 32) % 2 == h].tolist() for h in (0, 1)]
        for p in range(1, n):
            full_rows[b, p] += pools[(p // 32) % 2].pop() if place == "kept" else int(perm[p - 1])
    live = (torch.arange(Sq)[None, :] < torch.tensor(counts)[:, None]).reshape(-1).cuda()
    full_rows, qkv = full_rows.reshape(-1).cuda(), _full()["qkv"]
    q = qkv[:, :HD].index_select(0, full_rows).contiguous()
    return full_rows, live, q, qkv[:, HD:], torch.tensor(counts).int().cuda()  # K | V where they are


@pytest.mark.parametrize("place", ["kept", "random"])
@pytest.mark.parametrize("Sq,counts", CASES, ids=[f"Sq{s}-{'_'.join(map(str, c))}" for s, c in CASES])
def test_compact_rows_against_full_packed_buffer(cuda, Sq, counts, place):
    O, f = torch.ops.dedloc, _full()
    rows, n, info = f["rows"], len(LENS), (f["seqinfo"], f["host"])
    full_rows, live, q, kv, qcnt = _plan(rows, Sq, counts, place)
    lr, cr = full_rows[live], torch.nonzero(live).squeeze(1)
    dout_c = torch.randn(n * Sq, HD, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3)).bfloat16()
    dout_f = torch.zeros(rows[-1], HD, device=cuda, dtype=torch.bfloat16)
    dout_f[lr] = dout_c[cr]  # the dead rows' dout must be ignored
    db_c, db_f = torch.full((3 * HD,), 0.25, device=cuda), torch.full((3 * HD,), 0.25, device=cuda)
    out_c, lse_c = O.attn_varlen_fwd_q(q, kv, qcnt, *info, H, Sq, SCALE)
    dq_c, dkv_c, delta_c = O.attn_varlen_bwd_q(q, kv, qcnt, *info, out_c, dout_c, lse_c, H, Sq, SCALE, db_c)
    dqkv_f = O.attn_varlen_bwd(f["qkv"], *info, f["out"], dout_f, f["lse"], H, SCALE, db_f)
    ref_in = (q.float().cpu(), kv.float().cpu(), qcnt.cpu(), f["host"], f["host"])  # reference: the CPU op in fp32
    r_out, r_lse = O.attn_varlen_fwd_q(*ref_in, H, Sq, SCALE)
    r_db = torch.zeros(3 * HD)
    r_dq, r_dkv, _ = O.attn_varlen_bwd_q(*ref_in, r_out, dout_c.float().cpu(), r_lse, H, Sq, SCALE, r_db)
    r_out, r_lse, r_dq, r_dkv, r_db = (t.cuda() for t in (r_out, r_lse, r_dq, r_dkv, r_db))
    lse_comp, lse_full = lse_c.permute(0, 2, 1).reshape(n * Sq, H)[cr], f["lse"].t()[lr]
    r_lse = r_lse.permute(0, 2, 1).reshape(n * Sq, H)[cr]
    # key rows past each length; every row of a sequence without queries
    past = torch.cat([torch.arange(rows[b] + (LENS[b] if counts[b] else 0), rows[b + 1]) for b in range(n)]).cuda()
    fig = dict(
        out_equal=torch.equal(out_c[cr], f["out"][lr]), lse_equal=torch.equal(lse_comp, lse_full),
        dq_equal=torch.equal(dq_c[cr], dqkv_f[lr, :HD]),
        dead_zero=bool((out_c[~live] == 0).all() and (dq_c[~live] == 0).all()), dkv_zero=bool((dkv_c[past] == 0).all()),
        delta_equal=torch.equal(delta_c.permute(0, 2, 1).reshape(n * Sq, H)[cr], _delta_replay(dout_c[cr], out_c[cr])),
        dbk_untouched=bool((db_c[HD:2 * HD] == 0.25).all()),
        out_c=rel(out_c[cr], r_out[cr]), out_f=rel(f["out"][lr], r_out[cr]),
        lse_c=rel(lse_comp, r_lse), lse_f=rel(lse_full, r_lse),
        dq_c=rel(dq_c[cr], r_dq[cr]), dq_f=rel(dqkv_f[lr, :HD], r_dq[cr]),
        dkv_c=rel(dkv_c, r_dkv), dkv_f=rel(dqkv_f[:, HD:], r_dkv), db_c=rel(db_c - 0.25, r_db), db_f=rel(db_f - 0.25, r_db))
    print(Sq, counts, place, fig)
    assert fig["dead_zero"] and fig["dkv_zero"] and fig["delta_equal"] and fig["dbk_untouched"], fig
    if place == "kept":
        assert fig["out_equal"] and fig["lse_equal"] and fig["dq_equal"], fig
    else:
        assert fig["out_c"] <= 1.5 * fig["out_f"] and fig["lse_c"] <= 1.5 * fig["lse_f"] + 1e-6, fig
        assert fig["dq_c"] <= 1.5 * fig["dq_f"], fig
    assert fig["dkv_c"] <= 1.5 * fig["dkv_f"] and fig["db_c"] <= 1.5 * fig["db_f"], fig


def test_repeatable_and_contract(cuda):
    """Two runs give the same bits; layouts the kernels do not serve are refused, not computed."""
    O, f = torch.ops.dedloc, _full()
    Sq, info = CASES[1][0], (f["seqinfo"], f["host"])
    _, _, q, kv, qcnt = _plan(f["rows"], Sq, CASES[1][1], "kept")
    a, b = (O.attn_varlen_fwd_q(q, kv, qcnt, *info, H, Sq, SCALE) for _ in range(2))
    # (lse is written for live rows only: row 0 of every sequence but the dummy tail)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][:-1, :, :1], b[1][:-1, :, :1])
    ga, gb = (O.attn_varlen_bwd_q(q, kv, qcnt, *info, a[0], a[0], a[1], H, Sq, SCALE, None) for _ in range(2))
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    with pytest.raises(RuntimeError, match="head_dim 64"):  # q + seqinfo at one head of 128
        O.attn_varlen_fwd_q(q, kv, qcnt, *info, 1, Sq, SCALE)
    with pytest.raises(RuntimeError, match="multiple of 64"):  # a slot of 96 rows
        O.attn_varlen_fwd_q(q[:len(LENS) * 96], kv, qcnt, *info, H, 96, SCALE)
