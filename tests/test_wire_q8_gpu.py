"""BLOCKWISE_8BIT wire compression, GPU tier: the HIP kernels of csrc/kernels/comm_q8.hip against the
plain-torch operators on the same inputs and against the analytic bounds, with the fp32 side 0 to 3
elements past a 16-byte boundary (both load paths), and the segmented all-reduce end to end on one
GPU between two threads.
"""
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from wire_q8_checks import (QB, SENDERS, SIZES, block_amax, check_e2e, check_encoding, decode, make_values,
                            mean_bound, per_value, split, wire_bytes)

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc
SENTINEL = 12345.0


def _offset_copy(x, off, dev):
    """A device copy of ``x`` that starts ``off`` elements past a 16-byte boundary."""
    base = torch.full((x.numel() + 8,), SENTINEL, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    view = base[off:off + x.numel()]
    view.copy_(x)
    return view


def _untouched_around(view, off):
    """Nothing was written outside the view made by ``_offset_copy``."""
    base = torch.empty(0, dtype=torch.float32, device=view.device).set_(view.untyped_storage())
    outside = torch.cat([base[:off], base[off + view.numel():view.numel() + 8]])
    return bool(torch.all(outside == SENTINEL))


def _same_scales(a, b, tol=None):
    """Equal to one ulp (or ``tol``), NaN where the other is NaN."""
    nan = torch.isnan(a)
    assert torch.equal(nan, torch.isnan(b))
    tol = b.abs() * 2.0 ** -23 if tol is None else tol
    assert torch.all(((a - b).abs() <= tol)[~nan]), ((a - b).abs().max(), a, b)


def _cpu_pack(x):
    buf = torch.empty(wire_bytes(x.numel()), dtype=torch.uint8)
    OPS.pack_q8(x, buf)
    return buf


@pytest.mark.parametrize("n", SIZES)
def test_pack_q8_matches_the_cpu_operator(cuda, n):
    x = make_values(n, seed=n)
    want = _cpu_pack(x)
    ws, wc, _ = split(want, n)
    for off in range(4):
        buf = torch.full((wire_bytes(n),), 0xAB, dtype=torch.uint8, device=cuda)
        OPS.pack_q8(_offset_copy(x, off, cuda), buf)
        got = buf.cpu()
        check_encoding(got, x)  # layout, zero padding, the scale rule and the round-trip bound
        gs, gc, _ = split(got, n)
        _same_scales(gs, ws)
        assert int((gc.int() - wc.int()).abs().max()) <= 1
        assert torch.all((decode(got, n) - decode(want, n)).abs() <= per_value(torch.maximum(gs, ws), n))


@pytest.mark.parametrize("n", SIZES)
def test_unpack_q8_matches_the_cpu_operator(cuda, n):
    x = make_values(n, seed=n + 1)
    buf = _cpu_pack(x)
    want = decode(buf, n)
    base = torch.randn(n, generator=torch.Generator().manual_seed(n))
    dbuf = buf.to(cuda)
    for off in range(4):
        out = _offset_copy(torch.full((n,), 7.0), off, cuda)
        OPS.unpack_q8(dbuf, out, False)
        assert torch.equal(out.cpu(), want) and _untouched_around(out, off)
        acc = _offset_copy(base, off, cuda)
        OPS.unpack_q8(dbuf, acc, True)
        # the rounded product, then the sum: the same two roundings as the CPU operator
        assert torch.equal(acc.cpu(), base + want)
        assert _untouched_around(acc, off)


@pytest.mark.parametrize("k", SENDERS)
@pytest.mark.parametrize("n", SIZES)
def test_reduce_delta_q8_matches_the_cpu_operator_and_the_bound(cuda, n, k):
    masters = make_values(n, seed=100 * k + n, rows=k)
    weights = torch.rand(k, generator=torch.Generator().manual_seed(k)) + 0.1
    parts = torch.stack([_cpu_pack(m) for m in masters])
    want = torch.empty_like(parts)
    OPS.reduce_delta_q8(parts, weights, want, n)
    got = torch.full_like(parts, 0xCD, device=cuda)
    OPS.reduce_delta_q8(parts.to(cuda), weights.to(cuda), got, n)
    got = got.cpu()
    # the two sum the k terms of the fp32 average in different orders: (k + 2) roundings of values up
    # to 2 A_b in each, which moves a delta's block amax by that much and its scale by 1/127 of it
    a = block_amax(torch.stack([decode(p, n) for p in parts])).amax(0)
    slack = 2.0 * (k + 2) * 2.0 ** -23 * a
    for i in range(k):
        gs, gc, gpad = split(got[i], n)
        ws, wc, _ = split(want[i], n)
        assert int(gpad.abs().max()) == 0
        _same_scales(gs, ws, tol=ws.abs() * 2.0 ** -23 + slack / 127.0)
        assert int((gc.int() - wc.int()).abs().max()) <= 1
        step = per_value(torch.maximum(gs, ws), n)
        assert torch.all((decode(got[i], n) - decode(want[i], n)).abs() <= step + per_value(slack, n))
    # the analytic bound, on masters updated by the GPU's unpack (each at another alignment)
    new = []
    for i in range(k):
        m = _offset_copy(masters[i], i % 4, cuda)
        OPS.unpack_q8(got[i].to(cuda), m, True)
        new.append(m.cpu())
    mean, bound = mean_bound(masters, weights)
    ratio = ((torch.stack(new) - mean[None]).abs() / bound[None].clamp_min(1e-30)).max().item()
    print(f"n={n} k={k}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_special_blocks_on_the_gpu(cuda):
    n = 3 * QB + 40
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = make_values(n, seed=7)
        x[QB:2 * QB] = 0.0
        x[2 * QB + 5] = bad
        for off in (0, 1):
            buf = torch.full((wire_bytes(n),), 0xAB, dtype=torch.uint8, device=cuda)
            OPS.pack_q8(_offset_copy(x, off, cuda), buf)
            _assert_close_to_cpu(buf.cpu(), x)
            scales, codes, pad = split(buf, n)
            assert scales[1] == 0 and torch.all(codes[QB:2 * QB] == 0)
            assert torch.isnan(scales[2]) and torch.all(codes[2 * QB:3 * QB] == 0) and int(pad.abs().max()) == 0
            y = torch.zeros(n, device=cuda)
            OPS.unpack_q8(buf, y, False)
            y = y.cpu()
            assert torch.all(torch.isnan(y[2 * QB:3 * QB])) and torch.all(y[QB:2 * QB] == 0)
            for lo, hi in ((0, QB), (3 * QB, n)):
                assert torch.all((y[lo:hi] - x[lo:hi]).abs() <= 0.501 * per_value(scales, n)[lo:hi])
    # a sender with a NaN block poisons that block of every delta, and only that block
    masters = make_values(n, seed=8, rows=3)
    masters[1, 5] = float("nan")
    parts = torch.stack([_cpu_pack(m) for m in masters]).to(cuda)
    deltas = torch.empty_like(parts)
    OPS.reduce_delta_q8(parts, torch.ones(3, device=cuda), deltas, n)
    for i in range(3):
        d = decode(deltas[i], n)
        assert torch.all(torch.isnan(d[:QB])) and torch.all(torch.isfinite(d[QB:]))


def _assert_close_to_cpu(got, x):
    """Ties may round differently: scales to an ulp and codes within one of the CPU operator's."""
    n = x.numel()
    gs, gc, _ = split(got, n)
    ws, wc, _ = split(_cpu_pack(x), n)
    _same_scales(gs, ws)
    assert int((gc.int() - wc.int()).abs().max()) <= 1


@pytest.mark.parametrize("k", SENDERS)
def test_identical_rows_and_zero_weight_on_the_gpu(cuda, k):
    n = 4097
    parts = _cpu_pack(make_values(n, seed=3))[None].repeat(k, 1).to(cuda)
    deltas = torch.full_like(parts, 0xCD)
    OPS.reduce_delta_q8(parts, (torch.rand(k) + 0.1).to(cuda), deltas, n)
    assert int(deltas.max()) == 0
    parts = torch.stack([_cpu_pack(make_values(n, seed=10 + i)) for i in range(k)]).to(cuda)
    for w in (torch.zeros(k), -torch.ones(k)):
        deltas = torch.full_like(parts, 0xCD)
        OPS.reduce_delta_q8(parts, w.to(cuda), deltas, n)
        assert int(deltas.max()) == 0


def test_bindings_reject_wrong_sizes_and_misaligned_buffers(cuda):
    n = 1000
    x = torch.randn(n, device=cuda)
    with pytest.raises(RuntimeError):
        OPS.pack_q8(x, torch.empty(wire_bytes(n) + 16, dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError):
        OPS.pack_q8(x, torch.empty(wire_bytes(n) + 16, dtype=torch.uint8, device=cuda)[4:4 + wire_bytes(n)])
    with pytest.raises(RuntimeError):
        OPS.unpack_q8(torch.empty(wire_bytes(n), dtype=torch.uint8, device=cuda), torch.empty(n + 16, device=cuda))
    with pytest.raises(RuntimeError):
        parts = torch.zeros(65, wire_bytes(16), dtype=torch.uint8, device=cuda)
        OPS.reduce_delta_q8(parts, torch.ones(65, device=cuda), torch.empty_like(parts), 16)


@pytest.mark.parametrize("codecs", [["FLOAT16", "BLOCKWISE_8BIT"], "BLOCKWISE_8BIT"])
def test_two_members_end_to_end_on_one_gpu(cuda, codecs):
    check_e2e(cuda, codecs)
