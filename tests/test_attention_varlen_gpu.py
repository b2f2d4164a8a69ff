"""The variable-length (packed batch) fused attention kernels, called directly through
``torch.ops.dedloc.attn_varlen_fwd`` / ``attn_varlen_bwd`` at head_dim 64 and 128.

Layout under test (docs/KERNELS.md, "Packed variable-length batches"): sequence b owns the slot
rows[b] .. rows[b+1] of the token buffer, a slot holds round_up(len[b], 64) rows, seqinfo =
int32[2B + 1] (row offsets, then key lengths), lse / delta are [H, T].

Check 1: against an fp32 reference run sequence by sequence on the real rows only (the bounds of
         tests/test_attention_head128_gpu.py: out 1.5e-2, lse 1e-2, gradients 3e-2, bias gradient
         against the column sums 1e-4), exact zeros in dK / dV past each length and in the key part
         of the bias gradient.
Check 2: against the fixed-S kernels on the same sequences padded to S = 512 with kvinfo lengths and
         dout zeroed on non-real rows: per query row the tile sequence and the arithmetic are the
         same, so out, lse and dQ / dK / dV are compared with torch.equal on the real rows.
         Measured on an MI355X: bit-equal at head_dim 64 in every case and at head_dim 128 for the
         one-tile case; at head_dim 128 with more than one key tile NOT equal (forward output one
         bf16 step apart in 13 % of the elements, lse one fp32 step in 4 % of the rows).  Cause,
         found and confirmed on the GPU: the row maximum is taken by an inline-asm v_max3_f32
         (vmax3, dl_attn_tile.h) that reads the S = K Q^T accumulators right behind the MFMA chain
         that writes them; the compiler inserts the wait states an MFMA result needs before a
         VALU read for its own instructions but not for inline asm, so what the maximum sees
         depends on the instruction schedule, and the head_dim-128 forward is scheduled
         differently in its two instantiations (the packed one has no additive-bias path).  With
         wait states in front of the v_max3 the two are bit-equal (and the fixed-S kernel's own
         kvinfo and additive-bias forms, 41060 differing outputs of 131072 today, differ in 19).
         It is benign here: the deferred-rescale maximum is only a reference point within 2^8 of
         the true one, both results sit at the same distance from the fp32 reference.  Fixing
         vmax3 changes the fixed-S kernels and is left to a change of its own; as the check
         provides for this case, at head_dim 128 the difference is bounded by the fixed-S
         kernel's own distance to the fp32 reference on the same case, computed here.
Check 3: repeatability, a late spike that crosses the deferred-rescale threshold inside one short
         sequence, and the contract violations the bindings refuse.

Every case prints the figures it measured as one JSON line before it asserts."""
import functools
import json
import math
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 2
S_PAD = 512
MAIN = [1, 63, 64, 65, 200, 256, 257, 512]
random.Random(0).shuffle(MAIN)  # -> slot starts on every residue of 64 modulo 256 (asserted below)
LISTS = {"main": tuple(MAIN), "full": (512,), "one": (1,)}
OPS = None


@pytest.fixture(autouse=True)
def _ops(cuda):
    global OPS
    import dedloc_amd.ops  # noqa: F401

    OPS = torch.ops.dedloc


def rel(a, b, floor=0.0):
    a, b = a.float(), b.float()
    return ((a - b).norm() / max(b.norm().item(), floor, 1e-12)).item()


def _record(case, **figures):
    print(json.dumps({"case": case, **{k: (round(v, 8) if isinstance(v, float) else v) for k, v in figures.items()}}))


def _rows(lens):
    rows = [0]
    for n in lens:
        rows.append(rows[-1] + (n + 63) // 64 * 64)
    return rows


def _seqinfo(rows, lens, dev):
    host = torch.tensor(list(rows) + list(lens), dtype=torch.int32)
    return host.to(dev), host


def _ref_seq(qkv, D, dout):
    """fp32 reference for ONE unmasked sequence (its real rows): out [n, H*D], lse [H, n] (log2
    units), dQKV [n, 3*H*D]."""
    n = qkv.shape[0]
    qkv_r = qkv.float().detach().requires_grad_(True)
    x = qkv_r.reshape(1, n, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    o = F.scaled_dot_product_attention(q, k, v)
    o = o.permute(0, 2, 1, 3).reshape(n, H * D)
    with torch.no_grad():
        lse = torch.logsumexp(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(D), -1)[0] * math.log2(math.e)
    g = torch.autograd.grad(o, qkv_r, dout.float())[0]
    return o.detach(), lse, g


def _real_mask(rows, lens, dev):
    real = torch.zeros(rows[-1], dtype=torch.bool, device=dev)
    for b, n in enumerate(lens):
        real[rows[b]:rows[b] + n] = True
    return real


def _run_varlen(qkv, dout, rows, lens, D, prefill=0.25):
    dev = qkv.device
    si, si_h = _seqinfo(rows, lens, dev)
    scale = 1.0 / math.sqrt(D)
    out, lse = OPS.attn_varlen_fwd(qkv, si, si_h, H, scale)
    dbias = torch.full((3 * H * D,), prefill, device=dev)  # pre-filled: the kernels accumulate
    dqkv = OPS.attn_varlen_bwd(qkv, si, si_h, out, dout, lse, H, scale, dbias)
    return out, lse, dqkv, dbias


@functools.lru_cache(maxsize=None)
def _case(name, D, spike=False):
    """One packed problem with everything the checks share, computed once: inputs, the packed run,
    the fp32 per-sequence reference and the fixed-S run of the same sequences padded to 512."""
    lens = LISTS[name] if not spike else (200, 100)
    dev = torch.device("cuda")
    rows = _rows(lens)
    T = rows[-1]
    g = torch.Generator(device=dev).manual_seed(11 + D + len(lens))
    qkv = (torch.randn(T, 3 * H * D, device=dev, generator=g) * 1.5).bfloat16()
    if spike:  # key 150 of the first sequence: third key tile, after two tiles of ordinary scores
        qkv[rows[0] + 150, H * D:2 * H * D] *= 12
    real = _real_mask(rows, lens, dev)
    dout = torch.randn(T, H * D, device=dev, generator=g).bfloat16() * real[:, None]  # zero on filler rows
    out, lse, dqkv, dbias = _run_varlen(qkv, dout, rows, lens, D)
    torch.cuda.synchronize()
    # fp32 reference, sequence by sequence, real rows only
    r_out, r_lse, r_g = torch.zeros(T, H * D, device=dev), torch.zeros(H, T, device=dev), torch.zeros(T, 3 * H * D,
                                                                                                     device=dev)
    for b, n in enumerate(lens):
        sl = slice(rows[b], rows[b] + n)
        r_out[sl], r_lse[:, sl], r_g[sl] = _ref_seq(qkv[sl], D, dout[sl])
    # the fixed-S kernels on the same sequences, right-padded to S_PAD (rows past a slot: other random
    # data, masked as keys by the length and with zero dout as queries)
    B = len(lens)
    qkv_p = (torch.randn(B * S_PAD, 3 * H * D, device=dev, generator=g) * 1.5).bfloat16()
    dout_p = torch.zeros(B * S_PAD, H * D, device=dev, dtype=torch.bfloat16)
    for b in range(B):
        slot = rows[b + 1] - rows[b]
        qkv_p[b * S_PAD:b * S_PAD + slot] = qkv[rows[b]:rows[b + 1]]
        dout_p[b * S_PAD:b * S_PAD + slot] = dout[rows[b]:rows[b + 1]]
    kvinfo = torch.tensor(list(lens) + [1], dtype=torch.int32, device=dev)
    mbias = torch.where(torch.arange(S_PAD, device=dev)[None, :] < kvinfo[:B, None], 0.0, -1e30).float().contiguous()
    scale = 1.0 / math.sqrt(D)
    out_p, lse_p = OPS.attn_fwd(qkv_p, mbias, H, S_PAD, scale, kvinfo)
    dqkv_p = OPS.attn_bwd(qkv_p, mbias, out_p, dout_p, lse_p, H, S_PAD, scale, kvinfo, None)
    torch.cuda.synchronize()
    return dict(lens=lens, rows=rows, T=T, qkv=qkv, dout=dout, real=real, out=out, lse=lse, dqkv=dqkv, dbias=dbias,
                r_out=r_out, r_lse=r_lse, r_g=r_g, out_p=out_p, lse_p=lse_p, dqkv_p=dqkv_p)


def test_main_list_covers_every_slot_residue():
    assert sorted({r % 256 for r in _rows(LISTS["main"])[:-1]}) == [0, 64, 128, 192]
    assert sorted(_rows([n])[1] for n in LISTS["main"]) == [64, 64, 64, 128, 256, 256, 320, 512]


def _check_reference(case, c, D):
    HD = H * D
    real, lens, rows = c["real"], c["lens"], c["rows"]
    fig = {"out": rel(c["out"][real], c["r_out"][real]),
           "lse": (c["lse"][:, real] - c["r_lse"][:, real]).abs().max().item()}
    # A part whose reference is exactly zero has no relative error: dQ and dK of a one-token sequence
    # (dS = P (dP - delta) with dP = delta analytically).  The kernel's dP and delta are fp32 sums of
    # the same D products in different orders, apart by at most D * 2^-24 = 8e-6 of |dO||V|.  Such a
    # part is measured against 1e-3 of the whole reference gradient, so the 3e-2 bound allows 3e-5 of
    # it; the floor is three orders below any non-degenerate part's norm and changes nothing there.
    floor = 1e-3 * c["r_g"][real].norm().item()
    for part, name in enumerate(("dq", "dk", "dv")):
        sl = slice(part * HD, (part + 1) * HD)
        fig[name] = rel(c["dqkv"][real][:, sl], c["r_g"][real][:, sl], floor)
    fig["dbias_q_vs_colsum"] = rel(c["dbias"][:HD] - 0.25, c["dqkv"][:, :HD].float().sum(0), floor)
    fig["dbias_q_vs_ref"] = rel(c["dbias"][:HD] - 0.25, c["r_g"][:, :HD].sum(0), floor)
    fig["dbias_v_vs_colsum"] = rel(c["dbias"][2 * HD:] - 0.25, c["dout"].float().sum(0))
    _record(case, **fig)
    assert c["out"].shape == (c["T"], HD) and c["lse"].shape == (H, c["T"]) and c["dqkv"].shape == c["qkv"].shape
    assert torch.isfinite(c["out"].float()).all() and torch.isfinite(c["lse"]).all()  # filler rows included
    assert torch.isfinite(c["dqkv"].float()).all()
    assert fig["out"] < 1.5e-2, fig
    assert fig["lse"] < 1e-2, fig
    for name in ("dq", "dk", "dv"):
        assert fig[name] < 3e-2, fig
    assert fig["dbias_q_vs_colsum"] < 1e-4, fig
    assert fig["dbias_q_vs_ref"] < 3e-2, fig
    assert fig["dbias_v_vs_colsum"] < 1e-4, fig
    assert torch.equal(c["dbias"][HD:2 * HD], torch.full_like(c["dbias"][HD:2 * HD], 0.25))  # key part untouched
    for b, n in enumerate(lens):  # keys past the length inside each slot: exactly zero dK / dV
        if rows[b] + n < rows[b + 1]:
            assert c["dqkv"][rows[b] + n:rows[b + 1], HD:].abs().max().item() == 0.0, (b, n)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ["main", "full", "one"])
def test_against_fp32_reference(cuda, name, D):
    _check_reference(f"varlen_ref {name} D={D}", _case(name, D), D)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ["main", "full", "one", "spike"])
def test_equals_fixed_s_kernels(cuda, name, D):
    """Real rows of the packed run against the fixed-S kernels on the padded batch: bit-equal."""
    c = _case("main", D, True) if name == "spike" else _case(name, D)
    rows, lens = c["rows"], c["lens"]
    diff = {"out": 0.0, "lse": 0.0, "dqkv": 0.0}
    same = {"out": True, "lse": True, "dqkv": True}
    for b, n in enumerate(lens):
        v, p = slice(rows[b], rows[b] + n), slice(b * S_PAD, b * S_PAD + n)
        pairs = {"out": (c["out"][v], c["out_p"][p]), "lse": (c["lse"][:, v], c["lse_p"][b][:, :n]),
                 "dqkv": (c["dqkv"][v], c["dqkv_p"][p])}
        for k, (x, y) in pairs.items():
            same[k] = same[k] and torch.equal(x, y)
            diff[k] = max(diff[k], (x.float() - y.float()).abs().max().item())
    fig = {**{f"maxdiff_{k}": v for k, v in diff.items()}, **{f"equal_{k}": v for k, v in same.items()}}
    if D == 64 or all(same.values()):
        _record(f"varlen_vs_fixed {name} D={D}", **fig)
        assert same["out"] and same["lse"] and same["dqkv"], (same, diff)
        return
    # head_dim 128 (module docstring): packed-to-fixed-S distance <= the fixed-S kernel's own distance
    # to the fp32 reference, per quantity, in the metrics of check 1 — nothing here is a chosen constant
    HD, real = H * D, c["real"]
    fx = {k: torch.zeros_like(c[k]) for k in ("out", "lse", "dqkv")}  # fixed-S results in the packed layout
    for b, n in enumerate(lens):
        v, p = slice(rows[b], rows[b] + n), slice(b * S_PAD, b * S_PAD + n)
        fx["out"][v], fx["lse"][:, v], fx["dqkv"][v] = c["out_p"][p], c["lse_p"][b][:, :n], c["dqkv_p"][p]
    floor = 1e-3 * c["r_g"][real].norm().item()  # as in _check_reference
    pairs = {"out": (rel(c["out"][real], fx["out"][real]), rel(fx["out"][real], c["r_out"][real])),
             "lse": ((c["lse"][:, real] - fx["lse"][:, real]).abs().max().item(),
                     (fx["lse"][:, real] - c["r_lse"][:, real]).abs().max().item())}
    for part, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(part * HD, (part + 1) * HD)
        pairs[nm] = (rel(c["dqkv"][real][:, sl], fx["dqkv"][real][:, sl], floor),
                     rel(fx["dqkv"][real][:, sl], c["r_g"][real][:, sl], floor))
    for k, (d_pf, d_fr) in pairs.items():
        fig[f"{k}_packed_vs_fixed"], fig[f"{k}_fixed_vs_fp32"] = d_pf, d_fr
    _record(f"varlen_vs_fixed {name} D={D}", **fig)
    for k, (d_pf, d_fr) in pairs.items():
        assert d_pf <= d_fr, (k, d_pf, d_fr)


@pytest.mark.parametrize("D", [64, 128])
def test_repeatable(cuda, D):
    """Two runs are bit-identical: the forward and dQKV (plain stores, one writer per element; the
    bias gradient is accumulated with atomics and is left out)."""
    c = _case("main", D)
    out2, lse2, dqkv2, _ = _run_varlen(c["qkv"], c["dout"], c["rows"], c["lens"], D)
    assert torch.equal(c["out"], out2) and torch.equal(c["lse"], lse2)
    assert torch.equal(c["dqkv"], dqkv2)


@pytest.mark.parametrize("D", [64, 128])
def test_rescale_late_spike(cuda, D):
    """One key spikes (x12) in the third key tile of a 200-token sequence: the deferred rescale
    fires inside one short sequence, next to a sequence that never rescales after its first tile."""
    _check_reference(f"varlen_late_spike D={D}", _case("main", D, True), D)


def _call(rows, lens, d, dev, T=None):
    T = rows[-1] if T is None else T
    qkv = torch.randn(T, 3 * H * d, device=dev).bfloat16()
    si, si_h = _seqinfo(rows, lens, dev)
    return OPS.attn_varlen_fwd(qkv, si, si_h, H, 1.0 / math.sqrt(d))


@pytest.mark.parametrize("rows,lens,what", [
    ([0, 96, 192], [50, 60], "not a multiple of 64"),
    ([0, 64, 128], [0, 60], "outside 1 .."),
    ([0, 64, 128], [64, 65], "outside 1 .."),
])
def test_contract_violations_raise(cuda, rows, lens, what):
    with pytest.raises(RuntimeError) as e:
        _call(rows, lens, 64, cuda)
    assert what in str(e.value), str(e.value)
    qkv = torch.randn(rows[-1], 3 * H * 64, device=cuda).bfloat16()
    out = torch.zeros(rows[-1], H * 64, device=cuda).bfloat16()
    lse = torch.zeros(H, rows[-1], device=cuda)
    si, si_h = _seqinfo(rows, lens, cuda)
    with pytest.raises(RuntimeError) as e:
        OPS.attn_varlen_bwd(qkv, si, si_h, out, out, lse, H, 0.125, None)
    assert what in str(e.value), str(e.value)


def test_head_dim_32_raises(cuda):
    with pytest.raises(RuntimeError) as e:
        _call([0, 64], [64], 32, cuda)
    assert "supported head sizes are 64 and 128" in str(e.value), str(e.value)
