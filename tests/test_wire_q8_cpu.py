"""BLOCKWISE_8BIT wire compression, CPU tier: the codec contract of the plain-torch operators (the
oracle of the GPU tier and the data plane of gloo groups), per-tensor codecs over segments in the
all-reduce, two processes over gloo, the codec-signature check of the averager and the plumbing from
the command line down.
"""
import multiprocessing as mp
import time

import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from wire_q8_checks import (QB, SENDERS, SIZES, block_amax, check_e2e, check_encoding, code_offset, decode,
                            make_values, mean_bound, num_blocks, per_value, segment_bounds, split, wire_bytes,
                            within_mean_bound)

OPS = torch.ops.dedloc


def _pack(x):
    buf = torch.full((wire_bytes(x.numel()),), 0xAB, dtype=torch.uint8)  # stale bytes: padding must be written
    OPS.pack_q8(x, buf)
    return buf


def _unpack(buf, n, into=None):
    out = torch.zeros(n) if into is None else into
    OPS.unpack_q8(buf, out, into is not None)
    return out


# ----------------------------------------------------------------------------- codec contract
@pytest.mark.parametrize("n", SIZES)
def test_pack_q8_layout_and_round_trip(n):
    from dedloc_amd.ops._lib import q8_bytes

    x = make_values(n, seed=n)
    assert q8_bytes(n) == wire_bytes(n)
    buf = _pack(x)
    check_encoding(buf, x)
    y = _unpack(buf, n)
    assert torch.equal(y, decode(buf, n))
    base = torch.randn(n)
    assert torch.equal(_unpack(buf, n, into=base.clone()), base + y)


def test_pack_q8_special_blocks():
    n = 3 * QB + 40
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = make_values(n, seed=7)
        x[QB:2 * QB] = 0.0            # block 1: all zero
        x[2 * QB + 5] = bad           # block 2: one non-finite value
        buf = _pack(x)
        scales, codes, pad = split(buf, n)
        assert scales[1] == 0 and torch.all(codes[QB:2 * QB] == 0)
        assert torch.isnan(scales[2]) and int(pad.abs().max()) == 0
        y = _unpack(buf, n)
        assert torch.all(torch.isnan(y[2 * QB:3 * QB])) and torch.all(y[QB:2 * QB] == 0)
        # the neighbours are untouched: encoded as they are without the bad value
        for lo, hi in ((0, QB), (3 * QB, n)):
            assert torch.all((y[lo:hi] - x[lo:hi]).abs() <= 0.501 * per_value(scales, n)[lo:hi])
            assert torch.all(torch.isfinite(y[lo:hi]))


# ----------------------------------------------------------------------------- reduce + unpack
def _reduce(masters, weights, mutate=None):
    """pack every master, reduce, add each sender's delta to its master -> the new masters."""
    k, n = masters.shape
    parts = torch.stack([_pack(m) for m in masters])
    deltas = torch.full_like(parts, 0xCD)
    OPS.reduce_delta_q8(parts, weights, deltas, n)
    if mutate is not None:
        deltas = mutate(parts, deltas, n)
    new = masters.clone()
    for i in range(k):
        OPS.unpack_q8(deltas[i].contiguous(), new[i], True)
    return parts, deltas, new


@pytest.mark.parametrize("k", SENDERS)
@pytest.mark.parametrize("n", SIZES)
def test_reduce_delta_q8_meets_the_derived_bound(n, k):
    masters = make_values(n, seed=100 * k + n, rows=k)
    weights = torch.rand(k, generator=torch.Generator().manual_seed(k)) + 0.1
    parts, deltas, new = _reduce(masters, weights)
    mean, bound = mean_bound(masters, weights)
    ratio = ((new - mean[None]).abs() / bound[None].clamp_min(1e-30)).max().item()
    print(f"n={n} k={k}: worst error / bound = {ratio:.3f}")
    assert within_mean_bound(new, masters, weights), ratio
    for i in range(k):  # every delta row is a well-formed segment of its own
        _, codes, pad = split(deltas[i], n)
        assert int(pad.abs().max()) == 0 and int(codes.abs().max()) <= 127


@pytest.mark.parametrize("k", SENDERS)
def test_reduce_delta_q8_identical_rows_and_zero_weight(k):
    n = 4097
    row = _pack(make_values(n, seed=3))
    parts = row[None].repeat(k, 1)
    deltas = torch.full_like(parts, 0xCD)
    OPS.reduce_delta_q8(parts, torch.rand(k) + 0.1, deltas, n)
    assert int(deltas.max()) == 0  # byte-equal to zero: scales, codes and padding
    parts = torch.stack([_pack(make_values(n, seed=10 + i)) for i in range(k)])
    for w in (torch.zeros(k), -torch.ones(k)):
        deltas = torch.full_like(parts, 0xCD)
        OPS.reduce_delta_q8(parts, w, deltas, n)
        assert int(deltas.max()) == 0


def _mutant_inputs():
    """Senders a few quantisation steps apart (so their rounding errors are independent while the
    deltas stay small against the values) and uneven weights: the setting in which a coarse delta
    scale shows."""
    n, k = 10007, 3
    base = make_values(n, seed=5)
    spread = 0.05 * per_value(block_amax(base), n)
    masters = base[None] + spread[None] * torch.randn(k, n, generator=torch.Generator().manual_seed(6))
    return masters, torch.tensor([1.0, 6.0, 1.0])


def test_mutants_fail_the_bound():
    masters, weights = _mutant_inputs()
    _, _, new = _reduce(masters, weights)
    assert within_mean_bound(new, masters, weights)

    def scales_one_block_off(parts, deltas, n):
        out = deltas.clone()
        nb = num_blocks(n)
        sc = deltas[:, :4 * nb].contiguous().view(torch.float32)
        out[:, :4 * nb] = torch.roll(sc, 1, dims=1).contiguous().view(torch.uint8)
        return out

    def delta_on_the_senders_scale(parts, deltas, n):
        out = deltas.clone()
        nb, co = num_blocks(n), code_offset(n)
        for i in range(parts.shape[0]):
            d = decode(deltas[i], n)  # the delta as the real kernel resolved it (finer than any mutant)
            s_in = split(parts[i], n)[0]
            q = torch.round(d / per_value(s_in, n)).clamp(-127, 127).to(torch.int8)
            out[i, :4 * nb] = s_in.view(torch.uint8)
            out[i, co:co + n] = q.view(torch.uint8)
        return out

    for mutant in (scales_one_block_off, delta_on_the_senders_scale):
        _, _, bad = _reduce(masters, weights, mutate=mutant)
        assert not within_mean_bound(bad, masters, weights), mutant.__name__


# ----------------------------------------------------------------------------- segmentation
@pytest.mark.parametrize("codecs", [["FLOAT16", "BLOCKWISE_8BIT"], ["BLOCKWISE_8BIT", "BLOCKWISE_8BIT"],
                                    "BLOCKWISE_8BIT"])
def test_group_of_one_is_a_no_op_and_no_segment_spans_two_tensors(codecs, monkeypatch):
    from dedloc_amd.averaging.allreduce import GroupSpec, butterfly_allreduce

    a, b = make_values(1000, seed=1), make_values(777, seed=2) * 1e-4
    a0, b0 = a.clone(), b.clone()
    packed = []
    real = OPS.pack_q8

    def spy(src, dst):
        packed.append((src.untyped_storage().data_ptr(), src.storage_offset(), src.numel()))
        return real(src, dst)

    monkeypatch.setattr(torch.ops.dedloc, "pack_q8", spy)
    spec = GroupSpec(ranks=[0], part_sizes=[1777], weights=[1.0], contributes=[True], my_index=0)
    butterfly_allreduce([a, b], spec, codecs, comm=None)
    assert torch.equal(a, a0) and torch.equal(b, b0)
    eight_bit = [t for t, c in zip((a, b), [codecs] * 2 if isinstance(codecs, str) else codecs)
                 if c == "BLOCKWISE_8BIT"]
    assert len(packed) == len(eight_bit)
    for (storage, offset, numel), t in zip(packed, eight_bit):  # one whole tensor each, never across
        assert storage == t.untyped_storage().data_ptr() and offset == 0 and numel == t.numel()


def test_segments_are_parts_times_tensors():
    from dedloc_amd.averaging.allreduce import _segments

    sizes, parts = [1000, 777], [300, 0, 900, 577]
    segs = _segments(sizes, [0, 300, 300, 1200, 1777], ["FLOAT16", "BLOCKWISE_8BIT"])
    assert [(s.tensor, s.offset, s.n) for s in segs] == segment_bounds(sizes, parts)
    assert [(s.part, s.tensor, s.offset, s.n) for s in segs] == [(0, 0, 0, 300), (2, 0, 300, 700), (2, 1, 0, 200),
                                                                 (3, 1, 200, 577)]
    assert len(segs) <= 3 + len(sizes) - 1  # non-empty parts + tensors - 1
    assert all(s.codec == ("FLOAT16", "BLOCKWISE_8BIT")[s.tensor] for s in segs)


@pytest.mark.parametrize("codecs", [["FLOAT16", "BLOCKWISE_8BIT"], "BLOCKWISE_8BIT"])
def test_two_members_end_to_end_on_the_cpu_operators(codecs):
    """The GPU tier's end-to-end check on the plain-torch operators: two threads, a queue each way."""
    check_e2e(torch.device("cpu"), codecs)


# ----------------------------------------------------------------------------- two processes over gloo
def _gloo_worker(rank, world, dht_ep, rounds, q):
    try:
        torch.set_num_threads(1)
        import dedloc_amd.ops  # noqa: F401
        from dedloc_amd.averaging.allreduce import GroupSpec, butterfly_allreduce
        from dedloc_amd.dht import DHT
        from dedloc_amd.parallel import GroupCommunicators

        dht = DHT(initial_peers=[dht_ep], listen=False)
        comms = GroupCommunicators(dht, "q8", f"peer{rank}".encode(), torch.device("cpu"), timeout_s=60)
        g = torch.Generator().manual_seed(0)
        p = torch.randn(4096, generator=g) + 3.0  # same start on every peer
        p0 = p.clone()
        step = 2e-4 * p0.abs()                    # relative update 2e-4: about 1/40 of a quantisation step
        own = (1.0 + 0.5 * rank) * step
        gr = torch.Generator().manual_seed(rank + 1)
        g16, g8 = torch.randn(1000, generator=gr), torch.randn(3000, generator=gr) * 1e-3
        members = [(f"peer{r}".encode(), {"backend": "gloo", "comms": []}) for r in range(world)]
        comm, rank_of = comms.get(members, b"round-0")
        ranks = [rank_of[m] for m, _ in members]
        # one gradient round, two tensors with a codec each, the parts cut inside the 8-bit tensor
        spec = GroupSpec(ranks=ranks, part_sizes=[2500, 1500], weights=[1.0, 3.0], contributes=[True, True],
                         my_index=rank)
        a16, a8 = g16.clone(), g8.clone()
        butterfly_allreduce([a16, a8], spec, ["FLOAT16", "BLOCKWISE_8BIT"], comm=comm, timeout=30)
        spec = GroupSpec(ranks=ranks, part_sizes=[2048, 2048], weights=[1.0, 3.0], contributes=[True, True],
                         my_index=rank)
        for _ in range(rounds):
            p += own
            butterfly_allreduce([p], spec, "BLOCKWISE_8BIT", comm=comm, timeout=30)
        q.put({"rank": rank, "p": p.numpy(), "p0": p0.numpy(), "step": step.numpy(), "g16": g16.numpy(),
               "g8": g8.numpy(), "a16": a16.numpy(), "a8": a8.numpy()})
        comms.close()
        dht.shutdown()
    except Exception:  # noqa: BLE001
        import traceback

        q.put({"rank": rank, "error": traceback.format_exc()})


@pytest.mark.multiproc
@pytest.mark.timeout(240)
def test_8bit_averaging_over_gloo_keeps_small_updates_and_meets_the_bounds():
    from dedloc_amd.dht import DHT

    world, rounds = 2, 100
    root = DHT(listen_on="127.0.0.1:*")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, root.endpoint, rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=200) for _ in range(world)], key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=30)
    root.shutdown()
    for r in res:
        assert "error" not in r, r["error"]
        for key in list(r):
            if key != "rank":
                r[key] = torch.from_numpy(r[key])
    weights = torch.tensor([1.0, 3.0])
    # gradient round: the fp16 tensor as accurate as the FLOAT16 wire, the 8-bit tensor within the
    # per-block bound of each of its segments (blocks count from the segment's start)
    exp16 = (weights[0] * res[0]["g16"] + weights[1] * res[1]["g16"]) / weights.sum()
    g8 = torch.stack([res[0]["g8"], res[1]["g8"]])
    for i, r in enumerate(res):
        assert torch.allclose(r["a16"], exp16, rtol=2e-3, atol=2e-3)
    for tensor, lo, n in segment_bounds([1000, 3000], [2500, 1500]):
        if tensor == 1:
            new = torch.stack([res[0]["a8"][lo:lo + n], res[1]["a8"][lo:lo + n]])
            assert within_mean_bound(new, g8[:, lo:lo + n], weights), (lo, n)
    # parameter rounds: the weighted mean of the masters moves by the weighted mean update
    mean_update = (weights[0] * 1.0 + weights[1] * 1.5) / weights.sum() * res[0]["step"]
    expected_move = rounds * mean_update
    moved = (weights[0] * (res[0]["p"] - res[0]["p0"]) + weights[1] * (res[1]["p"] - res[1]["p0"])) / weights.sum()
    frac = (moved.sum() / expected_move.sum()).item()
    # the peers agree to one quantisation step of the block: half a step of each peer's own code plus
    # the delta's rounding (a delta is at most about a step, resolved to 1/127 of itself)
    step_b = per_value(torch.maximum(block_amax(res[0]["p"]), block_amax(res[1]["p"])), 4096) / 127.0
    apart = ((res[0]["p"] - res[1]["p"]).abs() / step_b).max().item()
    print(f"moved {frac:.5f} of the exact amount; peers {apart:.3f} steps apart")
    assert 0.97 < frac < 1.03, frac
    assert apart <= 1.02, apart


# ----------------------------------------------------------------------------- codec signature
def test_mismatched_codecs_fail_the_round_at_once(caplog):
    import logging
    import threading

    caplog.set_level(logging.WARNING, logger="dedloc_amd.averaging.averager")

    from dedloc_amd.averaging.averager import DecentralizedAverager
    from dedloc_amd.dht import DHT

    root = DHT(listen_on="127.0.0.1:*")
    dhts = [DHT(initial_peers=[root.endpoint], listen=False) for _ in range(2)]
    timeout = 60.0
    avgs = [DecentralizedAverager([torch.ones(500), torch.ones(300)], d, "sig", peer_id=f"peer{i}".encode(),
                                  target_group_size=2, averaging_expiration=10.0, averaging_timeout=timeout,
                                  compression=c, allow_state_sharing=False)
            for i, (d, c) in enumerate(zip(dhts, (["FLOAT16", "BLOCKWISE_8BIT"], "FLOAT16")))]
    out = {}

    def run(i):
        out[i] = avgs[i].step(weight=1.0, expected_group_size=2)

    t0 = time.monotonic()
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    elapsed = time.monotonic() - t0
    try:
        assert out == {0: None, 1: None}
        assert elapsed < timeout / 2, elapsed  # failed after matchmaking, not at the averaging timeout
        assert all(a.comms.created == 0 for a in avgs)
        named = [r.getMessage() for r in caplog.records
                 if "FLOAT16,BLOCKWISE_8BIT" in r.getMessage() and "FLOAT16,FLOAT16" in r.getMessage()]
        assert len(named) == 2, caplog.text  # each member names both signatures
        assert all(torch.all(t == 1) for a in avgs for t in a.averaged_tensors)
    finally:
        for a in avgs:
            a.shutdown()
        for d in dhts:
            d.shutdown()
        root.shutdown()


def test_signature_is_announced_and_missing_signature_is_compatible():
    from dedloc_amd.averaging.averager import DecentralizedAverager
    from dedloc_amd.dht import DHT

    root = DHT(listen_on="127.0.0.1:*")
    avg = DecentralizedAverager([torch.ones(8), torch.ones(8)], root, "sig2", peer_id=b"me",
                                compression=["FLOAT16", "BLOCKWISE_8BIT"], allow_state_sharing=False)
    try:
        info = avg._info(1.0, None, avg._codecs(None, avg.averaged_tensors))
        assert info["compression"] == "FLOAT16,BLOCKWISE_8BIT"
        assert avg._info(1.0, None, avg._codecs("BLOCKWISE_8BIT", [torch.ones(3)]))["compression"] == "BLOCKWISE_8BIT"
        with pytest.raises(ValueError):
            avg._codecs(None, [torch.ones(3)])  # two names for one tensor
    finally:
        avg.shutdown()
        root.shutdown()


# ----------------------------------------------------------------------------- plumbing
def test_optimizer_hands_the_averager_one_codec_per_tensor():
    from dedloc_amd.dht import DHT
    from dedloc_amd.optim.collaborative import CollaborativeOptimizer
    from dedloc_amd.optim.lamb import FusedLamb
    from dedloc_amd.utils.flat import FlatParams

    root = DHT(listen_on="127.0.0.1:*")
    made = []
    try:
        for kwargs, want in (
                (dict(compression_type="BLOCKWISE_8BIT", state_averaging_compression="FLOAT16"),
                 ["FLOAT16", "BLOCKWISE_8BIT"]),
                (dict(compression_type="BLOCKWISE_8BIT"), ["BLOCKWISE_8BIT", "BLOCKWISE_8BIT"]),
                (dict(), ["FLOAT16", "FLOAT16"])):
            flat = FlatParams(torch.nn.Linear(16, 8).named_parameters(), device=torch.device("cpu"), with_bf16=False)
            co = CollaborativeOptimizer(FusedLamb(flat, lr=1e-3), dht=root, prefix=f"plumb{len(made)}",
                                        target_batch_size=8, batch_size_per_step=4, start=False,
                                        listen_on="127.0.0.1:*", peer_id=b"me", **kwargs)
            made.append(co)
            assert co.averager.averaged_tensors[0] is flat.fp32 and co.averager.averaged_tensors[1] is flat.grad
            assert list(co.averager.compression) == want  # [params, grads]
    finally:
        for co in made:
            co.shutdown()
        root.shutdown()


def test_cli_flag_and_names():
    from transformers import HfArgumentParser

    from dedloc_amd.averaging.allreduce import resolve_compression
    from dedloc_amd.cli.arguments import CollaborativeOptimizerArguments

    (args,) = HfArgumentParser(CollaborativeOptimizerArguments).parse_args_into_dataclasses(
        ["--compression", "BLOCKWISE_8BIT", "--state_averaging_compression", "FLOAT16"])
    assert args.compression == "BLOCKWISE_8BIT" and args.state_averaging_compression == "FLOAT16"
    (args,) = HfArgumentParser(CollaborativeOptimizerArguments).parse_args_into_dataclasses([])
    assert args.compression == "FLOAT16" and args.state_averaging_compression is None
    for name in ("UNIFORM_8BIT", "QUANTILE_8BIT"):
        with pytest.raises(ValueError, match="BLOCKWISE_8BIT"):
            resolve_compression(name, 1)


def test_unsupported_codec_is_rejected_by_the_averager():
    from dedloc_amd.averaging.averager import DecentralizedAverager

    with pytest.raises(ValueError, match="BLOCKWISE_8BIT"):
        DecentralizedAverager([torch.ones(4)], None, "x", peer_id=b"me", compression="UNIFORM_8BIT")


def test_emulated_delay_uses_fractional_wire_bytes():
    from dedloc_amd.averaging.allreduce import wire_bytes_per_value

    assert wire_bytes_per_value(["FLOAT16", "FLOAT16"], [100, 50]) == 2.0
    n = 17_850_000
    b = wire_bytes_per_value(["BLOCKWISE_8BIT"], [n])
    assert b == wire_bytes(n) / n and 1.015 < b < 1.016
    assert abs(wire_bytes_per_value(["FLOAT16", "BLOCKWISE_8BIT"], [n, n]) - (2.0 + b) / 2) < 1e-12
