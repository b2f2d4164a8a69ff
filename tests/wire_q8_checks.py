"""Shared checks of the BLOCKWISE_8BIT wire codec (tests/test_wire_q8_cpu.py, tests/test_wire_q8_gpu.py).

Everything here works on host tensors and from the wire format alone (blocks of 256 values from the
segment's start, fp32 scales at byte 0, int8 codes from round_up(4 nb, 16), padding 0)."""
import torch

QB = 256
SIZES = (1, 15, 16, 255, 256, 257, 4097, 10007)
SENDERS = (1, 3, 20)


def round_up(a, m):
    return (a + m - 1) // m * m


def num_blocks(n):
    return (n + QB - 1) // QB


def code_offset(n):
    return round_up(4 * num_blocks(n), 16)


def wire_bytes(n):
    return code_offset(n) + round_up(n, 16)


def split(buf, n):
    """(scales fp32 [nb], codes int8 [n], padding bytes) of one encoded segment."""
    buf = buf.detach().cpu().reshape(-1)
    nb, co = num_blocks(n), code_offset(n)
    scales = buf[:4 * nb].clone().view(torch.float32)
    codes = buf[co:co + n].clone().view(torch.int8)
    pad = torch.cat([buf[4 * nb:co], buf[co + n:]])
    return scales, codes, pad


def per_value(block_values, n):
    """[..., nb] -> [..., n]: each block's value repeated over its elements."""
    return block_values.repeat_interleave(QB, dim=-1)[..., :n]


def block_amax(x):
    """[..., n] -> [..., nb]: max |x| of each block."""
    n = x.shape[-1]
    nb = num_blocks(n)
    padded = torch.nn.functional.pad(x.abs(), (0, nb * QB - n))
    return padded.reshape(*x.shape[:-1], nb, QB).amax(-1)


def decode(buf, n):
    scales, codes, _ = split(buf, n)
    return codes.float() * per_value(scales, n)


def make_values(n, seed, rows=None):
    """randn with every block scaled by its own factor from 1e-3 to 1e2."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if rows is None else (rows, n)
    mag = 10.0 ** (torch.rand(num_blocks(n), generator=g) * 5.0 - 3.0)
    return torch.randn(shape, generator=g) * per_value(mag, n)


def check_encoding(buf, x):
    """Layout, scale rule and round-trip bound of one encoded segment of finite values ``x``."""
    x = x.detach().cpu().reshape(-1)
    n = x.numel()
    assert buf.dtype == torch.uint8 and buf.numel() == wire_bytes(n)
    scales, codes, pad = split(buf, n)
    assert int(pad.abs().max() if pad.numel() else 0) == 0, "padding bytes must be 0"
    want = block_amax(x) * torch.tensor(1.0 / 127.0)
    # the scale is amax / 127 in fp32 (one ulp: the two ways to round 1/127 and the product)
    assert torch.all((scales - want).abs() <= want * 2.0 ** -23), (scales, want)
    assert int(codes.abs().max()) <= 127
    err = (codes.float() * per_value(scales, n) - x).abs()
    assert torch.all(err <= 0.501 * per_value(scales, n)), float((err / per_value(scales, n).clamp_min(1e-30)).max())
    zero = per_value(scales, n) == 0
    assert torch.all(codes[zero] == 0)


def mean_bound(masters, weights):
    """(exact fp32 weighted mean [n], per-element bound [n]) for ``reduce_delta_q8`` followed by
    ``unpack_q8(add=True)``: 1.01 (2 A_b + D_b) / 254 with A_b the largest block amax over the
    senders and D_b the largest block amax of the exact deltas — half a step each for the sender's own
    code, the average and the delta code."""
    n = masters.shape[-1]
    w = weights.double()
    mean = ((masters.double() * w[:, None]).sum(0) / w.sum()).float()
    a = block_amax(masters).amax(0)
    d = block_amax(mean[None, :] - masters).amax(0)
    return mean, per_value(1.01 * (2.0 * a + d) / 254.0, n)


def within_mean_bound(new_masters, masters, weights):
    mean, bound = mean_bound(masters, weights)
    return bool(torch.all((new_masters - mean[None, :]).abs() <= bound[None, :]))


def segment_bounds(sizes, part_sizes, with_part=False):
    """[(tensor, offset in the tensor, n)] of the all-reduce's segments: parts x tensors (with_part:
    the reducing member as a fourth entry)."""
    out, starts = [], [0]
    for p in part_sizes:
        starts.append(starts[-1] + p)
    for j in range(len(part_sizes)):
        t0 = 0
        for t, n in enumerate(sizes):
            lo, hi = max(starts[j], t0), min(starts[j + 1], t0 + n)
            if hi > lo:
                out.append((t, lo - t0, hi - lo) + ((j,) if with_part else ()))
            t0 += n
    return out


class QueueComm:
    """Stand-in group communicator for members that are threads of one process: one queue per
    (source, destination) pair carries clones of the sent tensors (taken after the sender's stream
    has finished).  No RCCL, no gloo."""

    backend = "queues"

    def __init__(self, rank, queues, wait_s=30.0):
        self.rank, self.queues, self.wait_s = rank, queues, wait_s
        self.transfers = []  # (tag, peer, dtype, numel) of everything sent

    @staticmethod
    def _sync(t):
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()

    def p2p(self, sends, send_peers, recvs, recv_peers, deadline, tag=0):
        for t, peer in zip(sends, send_peers):
            self._sync(t)
            c = t.detach().clone()
            self._sync(c)
            self.transfers.append((tag, int(peer), t.dtype, t.numel()))
            self.queues[(self.rank, int(peer))].put((tag, c))
        for r, peer in zip(recvs, recv_peers):
            got_tag, c = self.queues[(int(peer), self.rank)].get(timeout=self.wait_s)
            assert got_tag == tag and c.dtype == r.dtype and c.shape == r.shape, (got_tag, tag, c.dtype, r.dtype,
                                                                                c.shape, r.shape)
            r.copy_(c)
            self._sync(r)


E2E_SIZES = (5000, 3001)
E2E_PARTS = (3000, 5001)     # the cut lies inside the first tensor
E2E_WEIGHTS = (1.0, 3.0)


def e2e_inputs(device):
    """Two members' tensors: a common value (the two tensors orders of magnitude apart, as parameters
    and gradients are) with a relative spread of 1e-3 between the members."""
    g = torch.Generator().manual_seed(0)
    base = [make_values(E2E_SIZES[0], seed=11), make_values(E2E_SIZES[1], seed=12) * 1e-3]
    return [[(b * (1.0 + 1e-3 * torch.randn(b.shape, generator=g))).to(device) for b in base] for _ in range(2)]


def e2e_round(tensors, codecs):
    """One ``butterfly_allreduce`` of the two members (a thread each) over a QueueComm, in place."""
    import queue
    import threading

    from dedloc_amd.averaging.allreduce import GroupSpec, butterfly_allreduce

    queues = {(a, b): queue.Queue() for a in range(2) for b in range(2) if a != b}
    comms = [QueueComm(r, queues) for r in range(2)]
    errors = []

    def member(rank):
        try:
            if tensors[rank][0].is_cuda:
                torch.cuda.set_device(tensors[rank][0].device)
            spec = GroupSpec(ranks=[0, 1], part_sizes=list(E2E_PARTS), weights=list(E2E_WEIGHTS),
                             contributes=[True, True], my_index=rank)
            butterfly_allreduce(tensors[rank], spec, codecs, comm=comms[rank], timeout=30)
            QueueComm._sync(tensors[rank][0])
        except Exception:  # noqa: BLE001
            import traceback

            errors.append(traceback.format_exc())

    threads = [threading.Thread(target=member, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(90)
    assert not errors, errors[0]
    assert not any(t.is_alive() for t in threads)
    return comms


def check_e2e(device, codecs):
    """Round 1 against the exact fp32 weighted mean (8-bit tensors: the per-block bound on each
    segment; others: the FLOAT16 tolerance), the wire traffic, and a second round on the averaged
    tensors, which moves an 8-bit tensor by at most one quantisation step of the block: the members
    are within a step of each other, so their codes differ by at most one, and a member moves by
    the others' share (here 3/4 at most) of that difference plus the delta's own rounding."""
    names = [codecs] * 2 if isinstance(codecs, str) else list(codecs)
    tensors = e2e_inputs(device)
    start = [[t.cpu().clone() for t in member] for member in tensors]
    comms = e2e_round(tensors, codecs)
    after1 = [[t.cpu().clone() for t in member] for member in tensors]
    w = torch.tensor(E2E_WEIGHTS)
    segs = segment_bounds(E2E_SIZES, E2E_PARTS)
    for t, name in enumerate(names):
        old = torch.stack([start[0][t], start[1][t]])
        new = torch.stack([after1[0][t], after1[1][t]])
        if name == "BLOCKWISE_8BIT":
            for tensor, lo, n in segs:
                if tensor == t:
                    mean, bound = mean_bound(old[:, lo:lo + n], w)
                    ratio = ((new[:, lo:lo + n] - mean[None]).abs() / bound[None].clamp_min(1e-30)).max().item()
                    print(f"{codecs}: tensor {t} segment at {lo}+{n}: worst error / bound = {ratio:.3f}")
                    assert ratio <= 1.0, (t, lo, n, ratio)
        else:
            mean = (old * w[:, None]).sum(0) / w.sum()
            assert torch.allclose(new, mean[None].expand_as(new), rtol=2e-3, atol=2e-3)
    # per pair and direction: the pair's segments and the fp32 weight out (tag 1), the deltas back (tag 2)
    for rank, comm in enumerate(comms):
        owned = segment_bounds(E2E_SIZES, E2E_PARTS, with_part=True)
        theirs = [(t, n) for t, lo, n, part in owned if part != rank]
        mine = [(t, n) for t, lo, n, part in owned if part == rank]
        size = lambda t, n: wire_bytes(n) if names[t] == "BLOCKWISE_8BIT" else n  # noqa: E731
        assert [x[3] for x in comm.transfers if x[0] == 1] == [size(t, n) for t, n in theirs] + [1]
        assert [x[3] for x in comm.transfers if x[0] == 2] == [size(t, n) for t, n in mine]
        assert [x[2] for x in comm.transfers if x[0] == 1][-1] == torch.float32
    e2e_round(tensors, codecs)
    for t, name in enumerate(names):
        if name != "BLOCKWISE_8BIT":
            continue
        for tensor, lo, n in segs:
            if tensor != t:
                continue
            a1 = torch.stack([after1[0][t][lo:lo + n], after1[1][t][lo:lo + n]])
            a2 = torch.stack([tensors[0][t].cpu()[lo:lo + n], tensors[1][t].cpu()[lo:lo + n]])
            step = per_value(block_amax(a1).amax(0), n) / 127.0
            moved = ((a2 - a1).abs() / step[None]).max().item()
            print(f"{codecs}: tensor {t} segment at {lo}+{n}: second round moved {moved:.3f} steps")
            assert moved <= 1.0, (t, lo, n, moved)

