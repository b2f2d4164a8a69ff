"""Butterfly all-reduce over a group communicator (RCCL on GPUs, gloo on CPU).

A matchmade group (any set of live peers) averages a list of flat fp32 tensors:

  1. pack   : wire = compress(x)                             (one HIP pack kernel per tensor)
  2. scatter: member j receives part j of everyone's wire    (one grouped send/recv, all pairs at once —
              on an 8-GPU xGMI mesh every GPU drives its 7 links concurrently instead of the one
              link per hop of a ring)
  3. reduce : avg_j = sum_k w_k wire_k[j] / sum_k w_k in fp32, and for every sender k the delta
              d_k[j] = compress(avg_j - decompress(wire_k[j]))     (one HIP reduce_delta kernel)
  4. return : member j sends d_k[j] back to sender k          (one grouped send/recv)
  5. unpack : x += decompress(d)                              (fp32, on the live tensor)

Returning averaged-part *deltas* (hivemind 0.9.x's ``averaged_part - tensor_part`` rule) instead of
the average keeps each peer's fp32 master tensor: the peer adds (average - what it sent), so the
compression residual of its own contribution stays in its fp32 tensor and parameter updates below
half a FLOAT16 ulp survive averaging (replacing the tensor by the decoded average would round the
master parameters to fp16 every global step).  When all peers hold the same tensor the deltas are
exactly zero.

Part sizes come from the load-balancing LP; client-mode members own no part (they only send and
receive), auxiliary members contribute no tensor (weight 0) but reduce a part.

Weights travel on the wire: each contributor sends its own fp32 weight (bit-exact, as 1-2 wire
elements) to every reducer together with the part, and the reducer reads the weights it applies
from what it received.  Only ``spec.weights[my_index]`` has to be known when the round starts — so
matchmaking can run ahead of the last micro-step of a global batch, before a peer knows how many
samples it will have contributed (``DecentralizedAverager.prejoin``) — and it may be a device scalar
(the count of finite samples, kept on the GPU), so the global step never waits for the host to
learn it.  A group whose weights sum to 0 leaves every tensor unchanged (zero deltas).

Codecs and segments: ``compression`` is one name for all tensors or one name per tensor.  When every
tensor uses the same NONE / FLOAT16 / BFLOAT16 the steps above run on one flat wire vector, as
described.  Otherwise (any BLOCKWISE_8BIT, or different codecs) they run per *segment*, the
intersection of one tensor with one member's part — at most #parts + #tensors - 1 of them — each
with its tensor's codec and its own buffers, each (pair, segment) one transfer of the same grouped
send/recv, the pair's fp32 weight one more (``float32[1]``); so no quantisation block ever spans two
tensors (parameters and gradients differ by orders of magnitude).  BLOCKWISE_8BIT encodes a segment
of n values in blocks of 256 counted from the segment's start (nb = ceil(n / 256), the last one may
be short) as ``uint8[round_up(4 nb, 16) + round_up(n, 16)]``: nb fp32 scales (max|x| / 127) at byte
0, then n int8 codes (rint(x / scale)) from byte round_up(4 nb, 16), padding bytes 0; a block with a
non-finite value has scale NaN and decodes to NaN as a whole.  A delta is encoded with its own
block scales (a delta block is small, so it is finely resolved), which is why 8 bits work without
error feedback; identical tensors still give exactly zero deltas.

Timeouts: completion is polled on the host against a deadline; on expiry the communicator is
aborted (``ncclCommAbort`` for RCCL) so the operations still posted on it can never be matched by a
later round, and the round raises ``AllreduceException``; the caller drops the communicator from its
cache (``parallel.GroupCommunicators.invalidate``).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import torch

from ..ops._lib import q8_bytes
from ..parallel.comm import CommError

WIRE_DTYPES = {"NONE": torch.float32, "FLOAT32": torch.float32, "FLOAT16": torch.float16,
               "BFLOAT16": torch.bfloat16}
BLOCKWISE_8BIT = "BLOCKWISE_8BIT"
CODECS = tuple(WIRE_DTYPES) + (BLOCKWISE_8BIT,)


class AllreduceException(CommError):
    pass


def resolve_compression(compression: Union[str, Sequence[str]], num_tensors: int) -> List[str]:
    """One codec name per tensor from a name or a per-tensor sequence of names."""
    names = [compression] * num_tensors if isinstance(compression, str) else list(compression)
    if len(names) != num_tensors:
        raise ValueError(f"{len(names)} compression names for {num_tensors} tensors")
    for name in names:
        if name not in CODECS:
            raise ValueError(f"unknown compression {name}; expected one of {sorted(CODECS)}")
    return names


def compression_signature(codecs: Sequence[str]) -> str:
    """What a member announces for a round: members with different signatures cannot average."""
    return ",".join(codecs)


def wire_bytes_per_value(codecs: Sequence[str], sizes: Sequence[int]) -> float:
    """Mean bytes on the wire per averaged value (fractional for 8 bits: the block scales)."""
    total = 0
    for name, n in zip(codecs, sizes):
        if name == BLOCKWISE_8BIT:
            total += q8_bytes(n) if n else 0
        else:
            total += n * torch.empty(0, dtype=WIRE_DTYPES[name]).element_size()
    return total / max(1, sum(sizes))


@dataclass
class GroupSpec:
    ranks: List[int]            # communicator rank of each member, in group order
    part_sizes: List[int]       # elements of the averaged vector owned by each member
    weights: List[float]        # averaging weight of each member (0 for auxiliary peers)
    contributes: List[bool]     # False for auxiliary peers (they send no tensor)
    my_index: int

    @property
    def size(self):
        return len(self.ranks)


def _p2p(comm, sends, send_peers, recvs, recv_peers, deadline, tag):
    if not sends and not recvs:
        return
    if comm is None:
        raise AllreduceException("a group of more than one member needs a communicator")
    try:
        comm.p2p(sends, send_peers, recvs, recv_peers, deadline, tag=tag)
    except CommError as e:
        raise AllreduceException(str(e)) from e


def butterfly_allreduce(tensors: Sequence[torch.Tensor], spec: GroupSpec,
                        compression: Union[str, Sequence[str]] = "FLOAT16", comm=None,
                        timeout: Optional[float] = 30.0, sources: Optional[Sequence[torch.Tensor]] = None):
    """Average ``tensors`` in place across the group described by ``spec``.

    ``compression``: a codec name, or one name per tensor.  ``sources``: pack these instead of
    ``tensors`` (same shapes) and add the averaging deltas to ``tensors`` — delayed parameter
    averaging packs a snapshot and collects the delta in a zeroed buffer while the live parameters
    keep training."""
    codecs = resolve_compression(compression, len(tensors))
    if len(set(codecs)) > 1 or codecs[0] == BLOCKWISE_8BIT:
        return _segmented_allreduce(tensors, spec, codecs, comm, timeout, sources)
    compression = codecs[0]
    ops = torch.ops.dedloc
    wire = WIRE_DTYPES[compression]
    dev = tensors[0].device
    sizes = [t.numel() for t in tensors]
    V = sum(sizes)
    assert sum(spec.part_sizes) == V, "part sizes must cover the averaged vector"
    me = spec.my_index
    starts = [0]
    for p in spec.part_sizes:
        starts.append(starts[-1] + p)
    my_lo, my_hi = starts[me], starts[me + 1]
    P = my_hi - my_lo
    contrib_idx = [j for j in range(spec.size) if spec.contributes[j]]
    if not contrib_idx:
        raise AllreduceException("group has no contributing member")
    deadline = time.monotonic() + timeout if timeout else None
    i_contribute = spec.contributes[me]
    # this contributor's weight as wire elements (the fp32 bits: 1 element of fp32, 2 of fp16/bf16)
    W = 4 // torch.empty(0, dtype=wire).element_size()
    w_me = spec.weights[me]
    if isinstance(w_me, torch.Tensor):  # a device scalar: the weight is never read on the host
        my_w = w_me.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous().view(wire)
    else:
        my_w = torch.tensor([float(w_me)], dtype=torch.float32).view(wire).to(dev)

    # 1. pack (compressed, unweighted: the reducer applies the weights in fp32)
    send = torch.empty(V if i_contribute else 0, dtype=wire, device=dev)
    if i_contribute:
        o = 0
        for t, n in zip(sources if sources is not None else tensors, sizes):
            ops.pack(t.reshape(-1), send[o:o + n], 1.0)
            o += n
    nc = len(contrib_idx)
    recv = torch.empty((max(1, nc), max(P, 1)), dtype=wire, device=dev)
    wrecv = torch.empty((max(1, nc), W), dtype=wire, device=dev)

    # 2. reduce-scatter: part j of every contributor's wire (and its weight) goes to member j (one
    #    grouped launch; the two transfers of a pair are matched in order)
    sends, send_peers, recvs, recv_peers = [], [], [], []
    for slot, j in enumerate(contrib_idx):
        if j == me:
            if P:
                recv[slot, :P].copy_(send[my_lo:my_hi])
                wrecv[slot].copy_(my_w)
            continue
        if P:
            recvs += [recv[slot, :P], wrecv[slot]]
            recv_peers += [spec.ranks[j]] * 2
    if i_contribute:
        for j in range(spec.size):
            if j != me and spec.part_sizes[j] > 0:
                sends += [send[starts[j]:starts[j + 1]], my_w]
                send_peers += [spec.ranks[j]] * 2
    _p2p(comm, sends, send_peers, recvs, recv_peers, deadline, tag=1)

    # 3. weighted fp32 average of my part and one delta row per contributor
    deltas = None
    if P:
        parts = recv if recv.shape[1] == P else recv[:, :P].contiguous()
        w = wrecv.view(torch.float32).reshape(-1)
        deltas = torch.empty_like(parts)
        ops.reduce_delta(parts, w, deltas)

    # 4. every contributor receives its deltas for every part
    dbuf = torch.empty(V if i_contribute else 0, dtype=wire, device=dev)
    sends, send_peers, recvs, recv_peers = [], [], [], []
    for slot, j in enumerate(contrib_idx):
        if j == me:
            if P:
                dbuf[my_lo:my_hi].copy_(deltas[slot])
            continue
        if P:
            sends.append(deltas[slot])
            send_peers.append(spec.ranks[j])
    if i_contribute:
        for j in range(spec.size):
            if j != me and spec.part_sizes[j] > 0:
                recvs.append(dbuf[starts[j]:starts[j + 1]])
                recv_peers.append(spec.ranks[j])
    _p2p(comm, sends, send_peers, recvs, recv_peers, deadline, tag=2)

    # 5. unpack: x += delta (auxiliary peers hold no averaged tensor)
    if i_contribute:
        o = 0
        for t, n in zip(tensors, sizes):
            ops.unpack(dbuf[o:o + n], t.reshape(-1), None, True)
            o += n


@dataclass(frozen=True)
class _Segment:
    part: int       # the member that reduces it
    tensor: int     # the tensor it lies in
    offset: int     # first element inside that tensor
    n: int          # elements
    codec: str

    def empty(self, rows: Optional[int], device) -> torch.Tensor:
        """A wire buffer of this segment, or ``rows`` of them."""
        if self.codec == BLOCKWISE_8BIT:
            width, dtype = q8_bytes(self.n), torch.uint8
        else:
            width, dtype = self.n, WIRE_DTYPES[self.codec]
        return torch.empty(width if rows is None else (rows, width), dtype=dtype, device=device)


def _segments(sizes: Sequence[int], part_starts: Sequence[int], codecs: Sequence[str]) -> List[_Segment]:
    """The non-empty intersections of parts and tensors, in vector order (part-major)."""
    segs, t0 = [], [0]
    for n in sizes:
        t0.append(t0[-1] + n)
    for j in range(len(part_starts) - 1):
        for t in range(len(sizes)):
            lo, hi = max(part_starts[j], t0[t]), min(part_starts[j + 1], t0[t + 1])
            if hi > lo:
                segs.append(_Segment(j, t, lo - t0[t], hi - lo, codecs[t]))
    return segs


def _segmented_allreduce(tensors, spec: GroupSpec, codecs: Sequence[str], comm, timeout, sources):
    """The same five steps with one codec per tensor: the unit of packing, transfer and reduction is
    a segment (one tensor x one member's part), so no quantisation block spans two tensors."""
    ops = torch.ops.dedloc
    dev = tensors[0].device
    sizes = [t.numel() for t in tensors]
    assert sum(spec.part_sizes) == sum(sizes), "part sizes must cover the averaged vector"
    me = spec.my_index
    starts = [0]
    for p in spec.part_sizes:
        starts.append(starts[-1] + p)
    contrib_idx = [j for j in range(spec.size) if spec.contributes[j]]
    if not contrib_idx:
        raise AllreduceException("group has no contributing member")
    deadline = time.monotonic() + timeout if timeout else None
    i_contribute = spec.contributes[me]
    segs = _segments(sizes, starts, codecs)
    mine = [s for s in segs if s.part == me]
    w_me = spec.weights[me]
    if isinstance(w_me, torch.Tensor):  # a device scalar: the weight is never read on the host
        my_w = w_me.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous()
    else:
        my_w = torch.tensor([float(w_me)], dtype=torch.float32).to(dev)

    def flat_slice(ts, s):
        return ts[s.tensor].reshape(-1)[s.offset:s.offset + s.n]

    # 1. pack every segment (compressed, unweighted: the reducer applies the weights in fp32)
    sent = {}
    if i_contribute:
        for s in segs:
            buf = sent[s] = s.empty(None, dev)
            src = flat_slice(sources if sources is not None else tensors, s)
            if s.codec == BLOCKWISE_8BIT:
                ops.pack_q8(src, buf)
            else:
                ops.pack(src, buf, 1.0)
    nc = len(contrib_idx)
    recv = [s.empty(nc, dev) for s in mine]
    wrecv = torch.empty((nc, 1), dtype=torch.float32, device=dev)

    # 2. reduce-scatter: a contributor's segments of part j, then its weight, go to member j (one
    #    grouped launch; the transfers of a pair are matched in order)
    sends, send_peers, recvs, recv_peers = [], [], [], []
    for slot, j in enumerate(contrib_idx):
        if j == me:
            for s, r in zip(mine, recv):
                r[slot].copy_(sent[s])
            if mine:
                wrecv[slot].copy_(my_w)
            continue
        if mine:
            recvs += [r[slot] for r in recv] + [wrecv[slot]]
            recv_peers += [spec.ranks[j]] * (len(mine) + 1)
    if i_contribute:
        for j in range(spec.size):
            theirs = [sent[s] for s in segs if s.part == j]
            if j != me and theirs:
                sends += theirs + [my_w]
                send_peers += [spec.ranks[j]] * (len(theirs) + 1)
    _p2p(comm, sends, send_peers, recvs, recv_peers, deadline, tag=1)

    # 3. weighted fp32 average of each of my segments and one delta row per contributor
    w = wrecv.reshape(-1)
    deltas = []
    for s, r in zip(mine, recv):
        d = torch.empty_like(r)
        if s.codec == BLOCKWISE_8BIT:
            ops.reduce_delta_q8(r, w, d, s.n)
        else:
            ops.reduce_delta(r, w, d)
        deltas.append(d)

    # 4. every contributor receives its deltas for every segment
    got = {}
    sends, send_peers, recvs, recv_peers = [], [], [], []
    for slot, j in enumerate(contrib_idx):
        if j == me:
            for s, d in zip(mine, deltas):
                got[s] = d[slot]
            continue
        sends += [d[slot] for d in deltas]
        send_peers += [spec.ranks[j]] * len(deltas)
    if i_contribute:
        for s in segs:
            if s.part != me:
                got[s] = s.empty(None, dev)
                recvs.append(got[s])
                recv_peers.append(spec.ranks[s.part])
    _p2p(comm, sends, send_peers, recvs, recv_peers, deadline, tag=2)

    # 5. unpack: x += delta (auxiliary peers hold no averaged tensor)
    if i_contribute:
        for s in segs:
            dst = flat_slice(tensors, s)
            if s.codec == BLOCKWISE_8BIT:
                ops.unpack_q8(got[s], dst, True)
            else:
                ops.unpack(got[s], dst, None, True)
