"""Padding-free batches: right-padded ``[B, S]`` collator output -> one packed token buffer.

The packed layout (the contract the attention / embedding kernels, the ops and the model share;
docs/KERNELS.md "Packed variable-length batches"):

  * sequence ``b`` of length ``len[b] >= 1`` owns the *slot* ``rows[b] .. rows[b + 1]`` of a token
    buffer of ``T`` rows; the slot holds ``round_up(len[b], 64)`` rows, so every slot starts on a
    multiple of 64 and no 64-row attention tile straddles two sequences;
  * the first ``len[b]`` rows of a slot are the real tokens, the rest are *filler*: pad token id,
    token type 0, positions continuing ``len[b], len[b] + 1, ...``, no labels.  Filler rows behave
    exactly as padded rows do in the rectangular layout: their keys are masked by the length, their
    outputs are finite and their upstream gradient is exactly zero;
  * ``seqinfo = int32[2B + 1]``: the ``B + 1`` row offsets followed by the ``B`` key lengths, on the
    device for the kernels and on the host (``seqinfo_host``) for the contract checks and the grids.

Tail: every GEMM entry point takes any multiple of 64 rows, but the weight gradients split their
reduction over the tokens into equal slices of whole 64-row tiles (``wgrad_splits8``,
csrc/bindings.cpp), and a ``T / 64`` with no useful divisor (302 = 2 x 151) leaves two thirds of the
chip idle in a third of the GEMM work.  So ``T`` is rounded up to ``tail_granule(T)`` rows (a power
of two, at most 1024 and at most T / 16: under 6.25 % extra rows) by a dummy tail of pad tokens:
one extra sequence, or two when the tail is longer than the batch's largest slot (the attention
grids are sized by the largest slot, so a 960-row dummy beside 512-row sequences would double
them).  A dummy's key length is its own slot size, so it attends to itself and stays finite; it
carries no labels, so its gradient contribution is exactly zero; ``seqinfo`` then holds ``B + 1``
(or ``B + 2``) sequences.
A zero-length sequence is never emitted (unwritten rows would poison the token reduction of the
weight gradients: 0 * NaN).

With host ``lengths`` (the CPU collators know them) packing launches a few gathers and no device
synchronisation.  Without them the lengths are read back from ``attention_mask``: ONE
synchronisation per batch, and a mask that is not a prefix mask raises ``ValueError``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

SLOT = 64  # slot granularity = the attention kernels' tile height


@dataclass
class PackedBatch:
    input_ids: torch.Tensor              # int64 [T]
    token_type_ids: Optional[torch.Tensor]  # int64 [T] (None when the batch had none)
    positions: torch.Tensor              # int32 [T]: offset of each row inside its slot
    seqinfo: torch.Tensor                # int32 [2B + 1] on the device: row offsets, then lengths
    seqinfo_host: torch.Tensor           # the same array in host memory
    row_start: torch.Tensor              # int64 [B] on the device: rows[b]
    src: torch.Tensor                    # int64 [T]: b * S + offset of the padded element a real row copies
    real: torch.Tensor                   # bool [T]: real token (not filler)
    lengths: List[int]                   # host, the B real sequences
    rows: List[int]                      # host, row offsets of every slot (the dummy tail's included)
    T: int
    max_slot: int                        # largest slot of a real sequence
    B: int                               # real sequences (seqinfo holds n_seq = B plus the dummy tail's)
    n_seq: int
    S: int                               # padded width of the batch this was packed from
    extras: Dict[str, torch.Tensor] = field(default_factory=dict)  # packed labels ([T], -100 on filler)

    @property
    def real_tokens(self) -> int:
        return sum(self.lengths)

    def pack_tokens(self, x: torch.Tensor, fill) -> torch.Tensor:
        """[B, S, ...] per-token values -> [T, ...]; filler rows get ``fill``."""
        flat = x.reshape((self.B * self.S,) + tuple(x.shape[2:])).index_select(0, self.src)
        real = self.real.view((-1,) + (1,) * (flat.dim() - 1))
        return torch.where(real, flat, torch.full_like(flat, fill))


def _lengths_from_mask(attention_mask: torch.Tensor) -> List[int]:
    am = attention_mask.bool()
    lens = am.sum(1)
    prefix = (am == (torch.arange(am.shape[1], device=am.device)[None, :] < lens[:, None])).all()
    # the one device synchronisation of the lengths-free form
    host = torch.cat([lens.to(torch.int64), prefix.to(torch.int64).view(1)]).cpu().tolist()
    if not host[-1]:
        raise ValueError("pack_batch: attention_mask is not a prefix (right-padded) mask")
    return host[:-1]


def slot_rows(lengths: Sequence[int]) -> List[int]:
    """Row offsets ``rows[0 .. B]`` of the slots of sequences with these lengths."""
    rows = [0]
    for n in lengths:
        rows.append(rows[-1] + (int(n) + SLOT - 1) // SLOT * SLOT)
    return rows


def tail_granule(T: int) -> int:
    """``T`` is rounded up to a multiple of this many rows: the largest power of two <= T / 16, within
    64 .. 1024 (1024 rows = 16 reduction tiles: the split the full-length batches get)."""
    g = SLOT
    while g * 2 <= min(1024, T // 16):
        g *= 2
    return g


def make_seqinfo(lengths: Sequence[int], device, tail: bool = True):
    """(seqinfo on ``device``, its host copy, row offsets, key lengths) for these sequences, with the
    dummy tail sequence appended when ``tail`` and the row count needs one."""
    lens = [int(n) for n in lengths]
    rows = slot_rows(lens)
    if tail:
        g = tail_granule(rows[-1])
        extra = (rows[-1] + g - 1) // g * g - rows[-1]
        cap = max(rows[b + 1] - rows[b] for b in range(len(lens)))  # no dummy larger than a real slot
        while extra:
            n = min(extra, cap)
            rows.append(rows[-1] + n)
            lens.append(n)  # attends to itself: finite rows, no labels
            extra -= n
    host = torch.tensor(rows + lens, dtype=torch.int32)
    return host.to(device, non_blocking=True), host, rows, lens


@torch.no_grad()
def pack_batch(batch: Dict[str, torch.Tensor], lengths: Optional[Sequence[int]] = None,
               pad_token_id: int = 0) -> PackedBatch:
    """Pack a collator's right-padded dict (``input_ids``, ``token_type_ids``, ``attention_mask``, and
    ``labels`` [B, S] when present).  ``mlm_positions`` / ``mlm_labels`` need no packing: the model
    turns (b, position) into ``rows[b] + position``."""
    ids = batch["input_ids"]
    B, S = ids.shape
    dev = ids.device
    if lengths is None:
        am = batch.get("attention_mask")
        lengths = [S] * B if am is None else _lengths_from_mask(am)
    lengths = [int(n) for n in lengths]
    if len(lengths) != B:
        raise ValueError(f"pack_batch: {len(lengths)} lengths for a batch of {B}")
    if any(n < 1 or n > S for n in lengths):
        raise ValueError(f"pack_batch: every length must be in 1 .. {S} (a zero-length sequence cannot be packed)")
    seqinfo, seqinfo_host, rows, seq_lens = make_seqinfo(lengths, dev)
    T, n_seq = rows[-1], len(seq_lens)
    slots = torch.tensor([rows[b + 1] - rows[b] for b in range(n_seq)])
    seq = torch.repeat_interleave(torch.arange(n_seq), slots)
    off = torch.arange(T) - torch.tensor(rows[:-1])[seq]
    real_h = (off < torch.tensor(seq_lens)[seq]) & (seq < B)  # the dummy tail is filler throughout
    src_h = torch.where(real_h, seq * S + off, torch.zeros_like(off))
    off = torch.where(seq < B, off, off % SLOT)  # the tail may be longer than the position table
    src = src_h.to(dev, non_blocking=True)
    real = real_h.to(dev, non_blocking=True)
    positions = off.to(torch.int32).to(dev, non_blocking=True)
    row_start = torch.tensor(rows[:B], dtype=torch.long).to(dev, non_blocking=True)
    pk = PackedBatch(input_ids=ids, token_type_ids=None, positions=positions, seqinfo=seqinfo,
                     seqinfo_host=seqinfo_host, row_start=row_start, src=src, real=real, lengths=lengths, rows=rows,
                     T=T, max_slot=int(slots[:B].max()), B=B, n_seq=n_seq, S=S)
    pk.input_ids = pk.pack_tokens(ids, pad_token_id)
    tt = batch.get("token_type_ids")
    if tt is not None:
        pk.token_type_ids = pk.pack_tokens(tt, 0)
    lab = batch.get("labels")
    if lab is not None and lab.dim() == 2 and tuple(lab.shape) == (B, S):
        pk.extras["labels"] = pk.pack_tokens(lab, -100)
    return pk


def unpack_rows(x: torch.Tensor, packed: PackedBatch, S: Optional[int] = None) -> torch.Tensor:
    """[T, ...] per-row values -> [B, S, ...] (differentiable).  Position ``s`` of sequence ``b`` is
    row ``rows[b] + s``; positions past a sequence's slot (no row exists for them) are zero."""
    S = packed.S if S is None else S
    ar = torch.arange(S, device=x.device)[None, :]
    slot = (packed.seqinfo[1:packed.B + 1] - packed.seqinfo[:packed.B]).to(torch.long)[:, None]
    inside = ar < slot
    idx = torch.where(inside, packed.row_start[:, None] + ar, torch.zeros_like(ar))
    out = x.index_select(0, idx.reshape(-1)).reshape((packed.B, S) + tuple(x.shape[1:]))
    return out * inside.view((packed.B, S) + (1,) * (x.dim() - 1)).to(out.dtype)
