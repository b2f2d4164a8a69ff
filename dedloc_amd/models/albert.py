"""ALBERT for pre-training (MLM + sentence-order prediction) on dedloc kernels.

Parity target: HF ``AlbertForPreTraining`` as built by ``albert/run_trainer.py:56-70`` from the
``albert-large-v2`` config.  State-dict keys, shapes, initialisation and
the ``config.json`` / ``pytorch_model.bin`` checkpoint layout are identical to HF, so checkpoints
round-trip with ``transformers`` (tested against it in tests/test_albert_model.py).

MI355X-first execution (not a port of HF's module graph):
  * parameters live in one flat fp32 buffer (``FlatParams``); compute uses its bf16 mirror;
    Q/K/V weights are adjacent so the three projections run as ONE [3H, H] GEMM;
  * attention is the fused flash kernel over the packed QKV buffer (no head transposes);
  * residual add + LayerNorm, embedding gather + LayerNorm and gelu_new are fused HIP kernels;
  * the MLM head runs only on masked positions, and its decoder + softmax-CE is one fused pass;
  * every parameter gradient accumulates in fp32 directly in the flat gradient buffer.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import asdict, dataclass, field, fields
from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..data.packing import PackedBatch, pack_batch, unpack_rows
from ..utils.flat import FlatParams

NEG_BIG = -1.0e30


@dataclass
class AlbertConfig:
    vocab_size: int = 30000
    embedding_size: int = 128
    hidden_size: int = 4096
    num_hidden_layers: int = 12
    num_hidden_groups: int = 1
    num_attention_heads: int = 64
    intermediate_size: int = 16384
    inner_group_num: int = 1
    hidden_act: str = "gelu_new"
    hidden_dropout_prob: float = 0.0
    attention_probs_dropout_prob: float = 0.0
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    classifier_dropout_prob: float = 0.1
    num_labels: Optional[int] = None  # classification heads (HF writes it to config.json as well)
    pad_token_id: int = 0
    bos_token_id: int = 2
    eos_token_id: int = 3
    model_type: str = "albert"
    architectures: List[str] = field(default_factory=lambda: ["AlbertForPreTraining"])

    @classmethod
    def albert_large_v2(cls, **kw) -> "AlbertConfig":
        """The config the reference downloads at albert/arguments.py:97-99."""
        base = dict(vocab_size=30000, embedding_size=128, hidden_size=1024, num_hidden_layers=24,
                    num_hidden_groups=1, num_attention_heads=16, intermediate_size=4096, inner_group_num=1)
        base.update(kw)
        return cls(**base)

    @classmethod
    def albert_base_v2(cls, **kw) -> "AlbertConfig":
        """albert-base-v2 (HF model card sizes): 12 x 768, 12 heads of 64."""
        base = dict(vocab_size=30000, embedding_size=128, hidden_size=768, num_hidden_layers=12,
                    num_hidden_groups=1, num_attention_heads=12, intermediate_size=3072, inner_group_num=1)
        base.update(kw)
        return cls(**base)

    @classmethod
    def albert_xxlarge_v2(cls, **kw) -> "AlbertConfig":
        """albert-xxlarge-v2 (= transformers.AlbertConfig's defaults): 12 x 4096, 64 heads of 64."""
        base = dict(vocab_size=30000, embedding_size=128, hidden_size=4096, num_hidden_layers=12,
                    num_hidden_groups=1, num_attention_heads=64, intermediate_size=16384, inner_group_num=1)
        base.update(kw)
        return cls(**base)

    @classmethod
    def albert_xlarge_v2(cls, **kw) -> "AlbertConfig":
        """albert-xlarge-v2 (HF model card sizes): 24 x 2048, 16 heads of 128 — its attention runs
        the fused head_dim-128 flash kernels (ops.FUSED_HEAD_DIMS; the composed path,
        ops.attn_composed_fwd / _bwd, serves head sizes outside that tuple)."""
        base = dict(vocab_size=30000, embedding_size=128, hidden_size=2048, num_hidden_layers=24,
                    num_hidden_groups=1, num_attention_heads=16, intermediate_size=8192, inner_group_num=1)
        base.update(kw)
        return cls(**base)

    BUILTIN = {"albert-large-v2": "albert_large_v2", "albert-base-v2": "albert_base_v2",
               "albert-xlarge-v2": "albert_xlarge_v2", "albert-xxlarge-v2": "albert_xxlarge_v2"}

    @classmethod
    def tiny(cls, **kw) -> "AlbertConfig":
        base = dict(vocab_size=512, embedding_size=64, hidden_size=128, num_hidden_layers=3, num_hidden_groups=1,
                    num_attention_heads=2, intermediate_size=256, max_position_embeddings=128)
        base.update(kw)
        return cls(**base)

    def to_dict(self) -> Dict:
        d = asdict(self)
        if d.get("num_labels") is None:  # HF's PretrainedConfig rejects num_labels=None
            d.pop("num_labels", None)
        return d

    @classmethod
    def from_dict(cls, d: Dict) -> "AlbertConfig":
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})

    @classmethod
    def from_pretrained(cls, path: str) -> "AlbertConfig":
        """Accepts a directory containing config.json, a json file, or the name 'albert-large-v2' /
        'albert-base-v2' / 'albert-xxlarge-v2' (or the reference-style S3 URL of such a config —
        there is no network, so it maps to the built-in copy)."""
        for name, ctor in cls.BUILTIN.items():
            if path == name or (isinstance(path, str) and path.endswith(f"{name}-config.json")
                                and not os.path.exists(path)):
                return getattr(cls, ctor)()
        if os.path.isdir(path):
            path = os.path.join(path, "config.json")
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def save_pretrained(self, directory: str):
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)


def _layer_prefix(g: int, i: int) -> str:
    return f"albert.encoder.albert_layer_groups.{g}.albert_layers.{i}."


# Schedule switches (module constants, not environment knobs: the tests flip all three in-process,
# bench/ab_step.py the first two).
# The backward's data-gradient GEMMs (dX = dY W) run against transposed weight copies made once per
# encoder call (the 24 layers share them): gemm8 with both operands K-inner beats the K-outer-B form
# by 5-10% on these shapes (profiles/gemm8_asm_dma_layouts_T131072.log).
_DGRAD_WT = True
# Weight gradients of the shared layer keep their token-split fp32 slabs across the layer
# applications and add them into the flat gradient once, at the last backward call
# (gemm_acc_f32_shared).
_SHARED_WGRAD = True
# AlbertForPreTraining reads only the MLM target rows and one [CLS] row per sequence of the last
# layer's output, so its last layer application runs on those rows alone (K and V still on every
# row): _AlbertLastLayerFn over ops.attn_fwd_q / attn_bwd_q.  Head_dim 64 on rectangular batches;
# everything else, and every other model class, runs the full layer.
_LAST_LAYER_ROWS = True


class _AlbertLayerFn(torch.autograd.Function):
    """One application of the shared ALBERT transformer layer with a hand-scheduled backward.

    fwd: qkv = h Wqkv^T + b (one GEMM) -> flash attention -> dense -> LN(. + h) -> ffn -> gelu_new
         -> ffn_output -> LN(. + h1)
    bwd: every weight gradient accumulates in fp32 into the flat gradient buffer (beta = 1 GEMMs),
         and both residual-branch gradient sums are folded into the dgrad GEMMs (C = ds + dY W),
         so the layer backward launches no standalone elementwise adds.
    """

    @staticmethod
    def forward(ctx, h, mask, lv, H, S, eps):
        O = ops.OPS
        qkv = O.gemm(h, lv["wqkv"], lv["bqkv32"], None, False, True, 0)
        scale = 1.0 / math.sqrt(qkv.shape[1] // (3 * H))
        if isinstance(mask, PackedBatch):  # packed variable-length batch: h is [T, hidden], S is unused
            att, lse = ops.attn_varlen_fwd(qkv, mask, H, scale)
        else:
            mbias, kvinfo = mask
            att, lse = ops.attn_fwd(qkv, mbias, H, S, scale, kvinfo)
        out, saved = _post_attention_fwd(O, att, h, lv, eps)
        ctx.save_for_backward(h, qkv, att, lse, *saved)
        ctx.lv, ctx.mask, ctx.H, ctx.S, ctx.scale = lv, mask, H, S, scale
        return out

    @staticmethod
    def backward(ctx, dy):
        O = ops.OPS
        h, qkv, att, lse, *saved = ctx.saved_tensors
        lv, H = ctx.lv, ctx.H
        datt, ds1 = _post_attention_bwd(O, dy.contiguous(), att, saved, lv)
        # the QKV bias gradient rides in the attention backward (query: colsum dQ, value: colsum
        # datt, key: exactly zero — softmax is shift invariant), no separate column-sum pass
        if isinstance(ctx.mask, PackedBatch):
            dqkv = ops.attn_varlen_bwd(qkv, ctx.mask, att, datt, lse, H, ctx.scale, lv["gbqkv"])
        else:
            dqkv = ops.attn_bwd(qkv, ctx.mask[0], att, datt, lse, H, ctx.S, ctx.scale, ctx.mask[1], lv["gbqkv"])
        _wgrad(O, dqkv, h, lv, "gwqkv")
        dh = _dgrad(O, dqkv, lv, "wqkv", ds1)  # residual branch folded in
        return dh, None, None, None, None, None


class LastLayerRows:
    """The rows of the last layer's input that the heads read, in the compact layout of
    ``ops.attn_fwd_q``: sequence b owns a slot of ``Sq`` rows (a multiple of 64) of ``rows`` [B*Sq].
    Its [CLS] row comes first.  Every other row sits in the half (rows 0-31 or 32-63) of a 64-row
    tile that it occupies in its own sequence, halves filled in order of appearance: the attention
    forward gives a query row the same bits wherever it sits only as long as it keeps its 32-row
    sub-block within the wave, and the heads' inputs then equal the full layer's bit for bit.  (A
    sequence with more than Sq/2 rows of one half puts the excess into the other half's free places:
    still the right rows, one rounding step apart.)  Places left free hold the [CLS] row again, a
    valid index: they get a zero gradient, and past ``qcnt[b]`` (int32[B], one more than the last
    place in use) they are dead in attention.  ``head_rows`` / ``targets`` are the compact rows under
    the MLM head and their labels, in the order the full path feeds them to the head.  ``owner``
    [B*Sq] names, for every place, the first place that holds the same row (itself, unless the row
    is repeated): the backward folds the gradients of a repeated row into that place."""

    def __init__(self, rows, qcnt, Sq, head_rows, targets, owner):
        self.rows, self.qcnt, self.Sq, self.head_rows, self.targets = rows, qcnt, Sq, head_rows, targets
        self.owner = owner

    @staticmethod
    def _build(b_idx, s_pos, targets, B, Sp, Sq):
        """b_idx / s_pos [N]: sequence and position of every MLM row, grouped by sequence."""
        dev = b_idx.device
        # an entry at position 0 (a target on [CLS], or an unused entry of the fixed-shape form) shares
        # the [CLS] place: autograd then sums the heads' gradients of that row as it does on the full
        # output, before the layer's backward
        cls = s_pos == 0
        odd = (s_pos // 32) % 2
        even = (1 - odd) * (~cls).to(odd.dtype)
        zeros = torch.zeros(B, dtype=torch.long, device=dev)
        n_odd, n_even = zeros.scatter_add(0, b_idx, odd), zeros.scatter_add(0, b_idx, even)
        # rank inside (sequence, half): the running count less the count before the sequence; the
        # [CLS] row holds rank 0 of the even half
        r_odd = torch.cumsum(odd, 0) - 1 - (torch.cumsum(n_odd, 0) - n_odd)[b_idx]
        r_even = torch.cumsum(even, 0) - (torch.cumsum(n_even, 0) - n_even)[b_idx]
        rank = torch.where(odd == 1, r_odd, r_even)
        cap = Sq // 2
        fits = rank < cap
        others = torch.where(odd == 1, (n_even + 1)[b_idx], n_odd[b_idx])  # rows of the other half
        half = torch.where(fits, odd, even)
        rank = torch.where(fits, rank, others + rank - cap)
        place = torch.where(cls, torch.zeros_like(rank), 64 * (rank // 32) + 32 * half + rank % 32)
        head_rows = b_idx * Sq + place
        rows = (torch.arange(B, device=dev)[:, None] * Sp).expand(B, Sq).reshape(-1).clone()
        rows[head_rows] = b_idx * Sp + s_pos
        qcnt = torch.ones(B, dtype=torch.long, device=dev).scatter_reduce(0, b_idx, place + 1, "amax")
        places = torch.arange(B * Sq, device=dev)
        first = torch.full((B * Sp,), B * Sq, dtype=torch.long, device=dev).scatter_reduce(0, rows, places, "amin")
        return LastLayerRows(rows, qcnt.to(torch.int32), Sq, head_rows, targets, first[rows])

    @staticmethod
    def from_positions(mlm_positions, mlm_labels, Sp):
        """Fixed-shape targets [B, P]: every entry gets a place (an unused one points at position 0
        with label -100 and shares the [CLS] place).  No host synchronisation.  None when the slot would not be smaller than the sequence."""
        B, P = mlm_positions.shape
        Sq = (1 + P + 63) // 64 * 64
        if P == 0 or Sq >= Sp:
            return None
        b_idx = torch.arange(B, device=mlm_positions.device).repeat_interleave(P)
        return LastLayerRows._build(b_idx, mlm_positions.reshape(-1), mlm_labels.reshape(-1), B, Sp, Sq)

    @staticmethod
    def from_labels(labels, Sp):
        """HF ``labels`` [B, S] (-100 = ignore).  The per-sequence target counts are read on the host
        — the one synchronisation this form costs (it replaces that of ``nonzero``) — and size the
        slot.  None without any target or when the slot would not be smaller than the sequence."""
        B, S = labels.shape
        sel = labels != -100
        host = sel.sum(1).tolist()
        M, Sq = sum(host), (1 + max(host) + 63) // 64 * 64
        if M == 0 or Sq >= Sp:
            return None
        pos = torch.nonzero_static(sel.reshape(-1), size=M).squeeze(1)  # (b, position) order, no sync
        return LastLayerRows._build(pos // S, pos % S, labels.reshape(-1)[pos], B, Sp, Sq)


class _AlbertLastLayerFn(torch.autograd.Function):
    """The last application of the shared layer, computed for the rows in ``sel`` (LastLayerRows)
    only: [B*S, hidden] in, [B*Sq, hidden] out.  K and V are projected for every row, everything
    else — Q, the attention queries, the output projection, both LayerNorms and the FFN — for the
    compact rows, forward and backward.  Same kernels and the same hand schedule as _AlbertLayerFn;
    each live output row equals the full layer's row."""

    @staticmethod
    def forward(ctx, h, mask, lv, H, S, eps, sel):
        O = ops.OPS
        Hd = h.shape[1]
        mbias, kvinfo = mask
        scale = 1.0 / math.sqrt(Hd // H)
        kv = O.gemm(h, lv["wqkv"][Hd:], lv["bqkv32"][Hd:], None, False, True, 0)
        hq = h.index_select(0, sel.rows)
        q = O.gemm(hq, lv["wqkv"][:Hd], lv["bqkv32"][:Hd], None, False, True, 0)
        att, lse = ops.attn_fwd_q(q, kv, sel.qcnt, mbias, H, S, scale, kvinfo)
        out, saved = _post_attention_fwd(O, att, hq, lv, eps)
        ctx.save_for_backward(h, hq, q, kv, att, lse, *saved)
        ctx.lv, ctx.mask, ctx.H, ctx.S, ctx.sel, ctx.scale = lv, mask, H, S, sel, scale
        return out

    @staticmethod
    def backward(ctx, dy):
        O = ops.OPS
        h, hq, q, kv, att, lse, *saved = ctx.saved_tensors
        lv, sel = ctx.lv, ctx.sel
        Hd = h.shape[1]
        # This layer's reduction lengths (B*Sq, and B*S for K/V only) are not the other layers', so it
        # stays out of their shared slab series: its views carry no wg_first, and _wgrad accumulates
        # straight into the fp32 gradient (it is the first backward call; the layer before it opens
        # the series).
        datt, ds1 = _post_attention_bwd(O, dy.contiguous(), att, saved, lv)
        dq, dkv, _ = ops.attn_bwd_q(q, kv, sel.qcnt, ctx.mask[0], att, datt, lse, ctx.H, ctx.S, ctx.scale, ctx.mask[1],
                                    lv["gbqkv"])
        O.gemm_acc_f32(dq, hq, lv["gwqkv"][:Hd], True, False)
        O.gemm_acc_f32(dkv, h, lv["gwqkv"][Hd:], True, False)
        # Data gradient.  Every row gets its K / V part; a row the heads read gets, as in the full
        # layer, ds1 + [dQ | dK | dV] Wqkv from ONE GEMM (one rounding to bf16, not the sum of two
        # rounded parts) and replaces its K / V-only value.  A row held by several places (the
        # padding repeats the [CLS] row) has their dQ and ds1 folded into its first place, whose
        # result every one of them writes back: equal values, so the copy is well defined.
        dqo = torch.zeros_like(dq).index_add_(0, sel.owner, dq)
        ds1o = torch.zeros_like(ds1).index_add_(0, sel.owner, ds1)
        dcat = torch.cat([dqo, dkv.index_select(0, sel.rows)], 1)
        if "wqkvt" in lv:  # transposed copy; its K | V column block serves the rows the heads do not read
            dhq = O.gemm(dcat, lv["wqkvt"], None, ds1o, False, True, 0)
            dh = O.gemm(dkv, lv["wqkvt"][:, Hd:], None, None, False, True, 0)
        else:
            dhq = O.gemm(dcat, lv["wqkv"], None, ds1o, False, False, 0)
            dh = O.gemm(dkv, lv["wqkv"][Hd:], None, None, False, False, 0)
        dh.index_copy_(0, sel.rows, dhq.index_select(0, sel.owner))
        return dh, None, None, None, None, None, None


def _post_attention_fwd(O, att, res, lv, eps):
    """The half of the layer behind attention, on the rows of ``att``: output projection -> LN ->
    FFN-up with gelu_new -> FFN-down -> LN.  Both residual sums (``res``, the rows of the layer's
    input under ``att``, and h1) ride in the GEMM epilogues (C = residual, beta = 1), so each
    LayerNorm reads one tensor and writes one: 2 of 4 LN HBM passes removed.  The FFN-up epilogue
    stores f = gelu_new'(h) (bf16) for the backward instead of the pre-activation h: it shares the
    forward's exp2 / rcp, and the FFN-down data gradient's epilogue becomes one multiply instead of a
    second sigmoid evaluation per element (gemm_gelu_d / gemm_dmul, gemm8 DL_EPI_GELUD / DL_EPI_DMUL).
    Returns the layer's output and the tensors ``_post_attention_bwd`` needs."""
    s1 = O.gemm(att, lv["wo"], lv["bo32"], res, False, True, 0)
    h1, _, m1, r1 = O.layernorm_fwd(s1, None, lv["ln1g"], lv["ln1b"], eps)
    f, g = O.gemm_gelu_d(h1, lv["w1"], lv["b132"])
    s2 = O.gemm(g, lv["w2"], lv["b232"], h1, False, True, 0)
    out, _, m2, r2 = O.layernorm_fwd(s2, None, lv["ln2g"], lv["ln2b"], eps)
    return out, (s1, m1, r1, h1, f, g, s2, m2, r2)


def _post_attention_bwd(O, dy, att, saved, lv):
    """Backward of ``_post_attention_fwd``: (datt, ds1), the gradients of ``att`` and of the first
    residual sum (the caller folds ds1 into its input gradient).  Accumulates the weight and bias
    gradients of the four parameter groups behind attention."""
    s1, m1, r1, h1, f, g, s2, m2, r2 = saved
    # LN backward also accumulates colsum(ds) = the bias grad of the Linear that fed it
    ds2 = O.layernorm_bwd(dy, s2, lv["ln2g"], m2, r2, lv["gln2g"], lv["gln2b"], True, lv["gb2"])
    _wgrad(O, ds2, g, lv, "gw2")
    # dgrad * gelu'(h) + ffn bias grad, one kernel; against the transposed weight copy when the
    # views carry one (see _DGRAD_WT)
    df = O.gemm_dmul(ds2, lv["w2t"], f, lv["gb1"], True) if "w2t" in lv else O.gemm_dmul(ds2, lv["w2"], f, lv["gb1"])
    _wgrad(O, df, h1, lv, "gw1")
    dh1 = _dgrad(O, df, lv, "w1", ds2)  # residual branch folded in
    del df
    ds1 = O.layernorm_bwd(dh1, s1, lv["ln1g"], m1, r1, lv["gln1g"], lv["gln1b"], True, lv["gbo"])
    _wgrad(O, ds1, att, lv, "gwo")
    return _dgrad(O, ds1, lv, "wo", None), ds1


def _wgrad(O, dy, x, lv, name):
    """lv[name] += dY^T X; with the layer's position among the applications of its weights
    (``wg_first`` / ``wg_last``, set by encode) the slab sum is deferred to the last backward call.
    (Forking these GEMMs onto a side stream beside the memory-bound kernels measured 10% slower
    free-running and no gain paired; removed in round 4.)"""
    if "wg_first" in lv:
        O.gemm_acc_f32_shared(dy, x, lv[name], True, False, lv["wg_first"], lv["wg_last"])
    else:
        O.gemm_acc_f32(dy, x, lv[name], True, False)


def _dgrad(O, dy, lv, name, residual):
    """dX = dY W (+ residual), against W^T's forward-layout copy when the layer views carry one."""
    if name + "t" in lv:
        return O.gemm(dy, lv[name + "t"], None, residual, False, True, 0)
    return O.gemm(dy, lv[name], None, residual, False, False, 0)


@torch.no_grad()
def _with_transposed_weights(lv: Dict) -> Dict:
    lv = dict(lv)
    for name in ("wqkv", "wo", "w1", "w2"):
        lv[name + "t"] = lv[name].t().contiguous()
    return lv


class AlbertPreTrainedModel(nn.Module):
    """Shared ALBERT trunk (embeddings, mapping-in, the shared layer group(s), optional pooler) with
    HF-compatible parameter names, flat fp32/bf16 storage and the fused encoder forward.  Heads are
    added by the subclasses (pre-training, sequence / token classification)."""

    add_pooler = True
    # Run forward on a packed, padding-free token buffer (data/packing.py): set by the trainers'
    # --pack_sequences, or per call with forward(..., pack_sequences=True).  Off by default.
    pack_sequences = False

    def __init__(self, config: AlbertConfig):
        super().__init__()
        self.config = c = config
        self._p: Dict[str, nn.Parameter] = {}
        E, H, I, V = c.embedding_size, c.hidden_size, c.intermediate_size, c.vocab_size
        add = self._add
        add("albert.embeddings.word_embeddings.weight", V, E)
        add("albert.embeddings.position_embeddings.weight", c.max_position_embeddings, E)
        add("albert.embeddings.token_type_embeddings.weight", c.type_vocab_size, E)
        with torch.no_grad():
            self._p["albert.embeddings.word_embeddings.weight"][c.pad_token_id].zero_()
        add("albert.embeddings.LayerNorm.weight", E, init="ones")
        add("albert.embeddings.LayerNorm.bias", E, init="zeros")
        add("albert.encoder.embedding_hidden_mapping_in.weight", H, E)
        add("albert.encoder.embedding_hidden_mapping_in.bias", H, init="zeros")
        for g in range(c.num_hidden_groups):
            for i in range(c.inner_group_num):
                pre = _layer_prefix(g, i)
                add(pre + "full_layer_layer_norm.weight", H, init="ones")
                add(pre + "full_layer_layer_norm.bias", H, init="zeros")
                for n in ("query", "key", "value"):
                    add(pre + f"attention.{n}.weight", H, H)
                for n in ("query", "key", "value"):
                    add(pre + f"attention.{n}.bias", H, init="zeros")
                add(pre + "attention.dense.weight", H, H)
                add(pre + "attention.dense.bias", H, init="zeros")
                add(pre + "attention.LayerNorm.weight", H, init="ones")
                add(pre + "attention.LayerNorm.bias", H, init="zeros")
                add(pre + "ffn.weight", I, H)
                add(pre + "ffn.bias", I, init="zeros")
                add(pre + "ffn_output.weight", H, I)
                add(pre + "ffn_output.bias", H, init="zeros")
        if self.add_pooler:
            add("albert.pooler.weight", H, H)
            add("albert.pooler.bias", H, init="zeros")
        self._add_heads()
        self.flat: Optional[FlatParams] = None

    def _add(self, name, *shape, init="normal"):
        t = torch.empty(*shape)
        if init == "normal":
            t.normal_(0.0, self.config.initializer_range)
        elif init == "ones":
            t.fill_(1.0)
        else:
            t.zero_()
        p = nn.Parameter(t)
        self._p[name] = p
        self.register_parameter(name.replace(".", "__"), p)

    def _add_heads(self):
        pass

    # ------------------------------------------------------------------ parameters / checkpoints
    def hf_named_parameters(self):
        return list(self._p.items())

    def materialize(self, device=None) -> FlatParams:
        """Move parameters into the flat buffers on ``device`` (call once before training)."""
        device = torch.device(device) if device is not None else next(iter(self._p.values())).device
        for p in self._p.values():
            p.data = p.data.to(device)
        self.flat = FlatParams(self.hf_named_parameters(), device=device)
        return self.flat

    def hf_state_dict(self) -> Dict[str, torch.Tensor]:
        """state dict with exactly the HF model class's keys."""
        return {k: v.detach() for k, v in self._p.items()}

    @torch.no_grad()
    def load_hf_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        missing = [k for k in self._p if k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:5]}...")
        for k, p in self._p.items():
            if k in sd:
                p.data.copy_(sd[k].to(p.dtype))
        if self.flat is not None:
            self.flat.refresh_bf16()

    def save_pretrained(self, directory: str):
        os.makedirs(directory, exist_ok=True)
        self.config.save_pretrained(directory)
        # tied entries are stored as separate tensors, as HF's torch.save of the state dict does
        sd = {k: v.detach().float().cpu().contiguous().clone() for k, v in self.hf_state_dict().items()}
        torch.save(sd, os.path.join(directory, "pytorch_model.bin"))

    @classmethod
    def from_pretrained(cls, directory: str, strict: Optional[bool] = None, **config_overrides):
        """Load a checkpoint directory.  Head classes loading a pre-training checkpoint keep their
        freshly initialised head (HF behaviour), so ``strict`` defaults to True only for the class
        that wrote it (keys must all be present)."""
        cfg = AlbertConfig.from_pretrained(directory)
        for k, v in config_overrides.items():
            setattr(cfg, k, v)
        model = cls(cfg)
        sd_path = os.path.join(directory, "pytorch_model.bin")
        if os.path.exists(sd_path):
            sd = torch.load(sd_path, map_location="cpu", weights_only=True)
        else:
            from safetensors.torch import load_file

            sd = load_file(os.path.join(directory, "model.safetensors"))
        if strict is None:
            strict = all(k in sd for k in model._p if not k.startswith("albert."))
        model.load_hf_state_dict(sd, strict=strict)
        return model

    def resize_token_embeddings(self, n: int):
        """HF semantics: grow/shrink the (tied) vocabulary; new rows ~ N(0, init_range)."""
        c = self.config
        if n == c.vocab_size:
            return
        assert self.flat is None, "resize before materialize()"
        for key in ("albert.embeddings.word_embeddings.weight", "predictions.bias"):
            if key not in self._p:
                continue
            old = self._p[key].data
            new = torch.empty((n,) + tuple(old.shape[1:]))
            if key.endswith("weight"):
                new.normal_(0.0, c.initializer_range)
            else:
                new.zero_()
            k = min(n, old.shape[0])
            new[:k] = old[:k]
            self._p[key].data = new
        c.vocab_size = n

    def no_decay_names(self) -> List[str]:
        """Reference grouping (albert/run_trainer.py:74-84): names containing 'bias' or
        'LayerNorm.weight' get no weight decay (full_layer_layer_norm.weight *is* decayed — SURVEY App. C.2)."""
        return [n for n in self._p if any(nd in n for nd in ("bias", "LayerNorm.weight"))]

    # ------------------------------------------------------------------ forward
    def _layer_views(self, g: int, i: int):
        f = self.flat
        pre = _layer_prefix(g, i)
        H = self.config.hidden_size
        return dict(
            wqkv=f.span(f.bf16, pre + "attention.query.weight", pre + "attention.value.weight", (3 * H, H)),
            gwqkv=f.span(f.grad, pre + "attention.query.weight", pre + "attention.value.weight", (3 * H, H)),
            bqkv=f.span(f.bf16, pre + "attention.query.bias", pre + "attention.value.bias", (3 * H,)),
            bqkv32=f.span(f.fp32, pre + "attention.query.bias", pre + "attention.value.bias", (3 * H,)),
            bo32=f.p(pre + "attention.dense.bias"), b132=f.p(pre + "ffn.bias"), b232=f.p(pre + "ffn_output.bias"),
            gbqkv=f.span(f.grad, pre + "attention.query.bias", pre + "attention.value.bias", (3 * H,)),
            wo=f.w(pre + "attention.dense.weight"), gwo=f.g(pre + "attention.dense.weight"),
            bo=f.w(pre + "attention.dense.bias"), gbo=f.g(pre + "attention.dense.bias"),
            ln1g=f.p(pre + "attention.LayerNorm.weight"), ln1b=f.p(pre + "attention.LayerNorm.bias"),
            gln1g=f.g(pre + "attention.LayerNorm.weight"), gln1b=f.g(pre + "attention.LayerNorm.bias"),
            w1=f.w(pre + "ffn.weight"), gw1=f.g(pre + "ffn.weight"), b1=f.w(pre + "ffn.bias"), gb1=f.g(pre + "ffn.bias"),
            w2=f.w(pre + "ffn_output.weight"), gw2=f.g(pre + "ffn_output.weight"),
            b2=f.w(pre + "ffn_output.bias"), gb2=f.g(pre + "ffn_output.bias"),
            ln2g=f.p(pre + "full_layer_layer_norm.weight"), ln2b=f.p(pre + "full_layer_layer_norm.bias"),
            gln2g=f.g(pre + "full_layer_layer_norm.weight"), gln2b=f.g(pre + "full_layer_layer_norm.bias"),
        )

    def _albert_layer(self, h, lv, mask, S, last_rows=None):
        c = self.config
        if last_rows is not None:
            return _AlbertLastLayerFn.apply(h, mask, lv, c.num_attention_heads, S, c.layer_norm_eps, last_rows)
        return _AlbertLayerFn.apply(h, mask, lv, c.num_attention_heads, S, c.layer_norm_eps)

    def last_layer_rows_supported(self) -> bool:
        """Whether the last layer can run on compact rows (LastLayerRows): the module switch, one
        layer per group application and head_dim 64 (the only head size with compact-query attention
        kernels)."""
        c = self.config
        return _LAST_LAYER_ROWS and c.inner_group_num == 1 and c.hidden_size == 64 * c.num_attention_heads

    def _packed(self, pack_sequences, input_ids, attention_mask, token_type_ids, lengths, labels=None):
        """The PackedBatch of this call, or None when the call runs on the rectangular layout."""
        if not (self.pack_sequences if pack_sequences is None else pack_sequences):
            return None
        batch = {"input_ids": input_ids, "attention_mask": attention_mask, "token_type_ids": token_type_ids}
        if labels is not None:
            batch["labels"] = labels
        return pack_batch(batch, lengths, self.config.pad_token_id)

    def encode(self, input_ids=None, attention_mask=None, token_type_ids=None, packed: Optional[PackedBatch] = None,
               last_rows=None):
        """Returns (sequence_output [B*S', H] bf16, S') where S' is S padded to a multiple of 64; with
        ``packed`` the trunk runs on the packed token buffer and returns ([T, H] bf16, None).
        Only when the caller passes ``last_rows`` (a LastLayerRows built for this S'; rectangular
        batches, see ``last_layer_rows_supported``) does the last layer run on those rows alone: the
        output is then the compact [B*Sq, H] tensor."""
        assert self.flat is not None, "call model.materialize(device) first"
        c, f = self.config, self.flat
        if packed is not None:
            return self._encode_packed(packed), None
        B, S = input_ids.shape
        Sp = (S + 63) // 64 * 64
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if Sp != S:
            pad = Sp - S
            input_ids = F.pad(input_ids, (0, pad), value=c.pad_token_id)
            attention_mask = F.pad(attention_mask, (0, pad), value=0)
            if token_type_ids is not None:
                token_type_ids = F.pad(token_type_ids, (0, pad), value=0)
        assert Sp <= c.max_position_embeddings, "sequence longer than max_position_embeddings"
        am = attention_mask.bool()
        mbias = torch.where(am, 0.0, NEG_BIG).to(torch.float32).contiguous()
        # right-padded masks (the usual case) let the attention kernels skip padded key tiles: pass
        # the lengths plus an on-device "every row is a prefix mask" flag (no host sync)
        lens = am.sum(1, dtype=torch.int32)
        prefix = (am == (torch.arange(Sp, device=am.device) < lens[:, None])).all()
        kvinfo = torch.cat([lens, prefix.to(torch.int32).view(1)]).contiguous()
        mask = (mbias, kvinfo)
        emb = "albert.embeddings."
        x = ops.embed_layernorm(
            input_ids, token_type_ids, f.p(emb + "word_embeddings.weight"), f.p(emb + "position_embeddings.weight"),
            f.p(emb + "token_type_embeddings.weight"), f.p(emb + "LayerNorm.weight"), f.p(emb + "LayerNorm.bias"),
            grads=(f.g(emb + "word_embeddings.weight"), f.g(emb + "position_embeddings.weight"),
                   f.g(emb + "token_type_embeddings.weight"), f.g(emb + "LayerNorm.weight"),
                   f.g(emb + "LayerNorm.bias")),
            eps=c.layer_norm_eps)
        return self._layers(x, mask, Sp, last_rows), Sp

    def _encode_packed(self, packed: PackedBatch):
        c, f = self.config, self.flat
        assert packed.max_slot <= c.max_position_embeddings, "sequence longer than max_position_embeddings"
        D = c.hidden_size // c.num_attention_heads
        if D not in ops.FUSED_HEAD_DIMS:
            raise RuntimeError(f"dedloc_amd: pack_sequences needs a fused attention head size {ops.FUSED_HEAD_DIMS}, "
                               f"this model has head_dim {D}")
        emb = "albert.embeddings."
        x = ops.embed_layernorm_packed(
            packed.input_ids, packed.token_type_ids, packed.positions, f.p(emb + "word_embeddings.weight"),
            f.p(emb + "position_embeddings.weight"), f.p(emb + "token_type_embeddings.weight"),
            f.p(emb + "LayerNorm.weight"), f.p(emb + "LayerNorm.bias"),
            grads=(f.g(emb + "word_embeddings.weight"), f.g(emb + "position_embeddings.weight"),
                   f.g(emb + "token_type_embeddings.weight"), f.g(emb + "LayerNorm.weight"),
                   f.g(emb + "LayerNorm.bias")),
            eps=c.layer_norm_eps)
        return self._layers(x, packed, 0)

    def _layers(self, x, mask, Sp, last_rows=None):
        """Mapping-in GEMM and the shared layer group(s) over a [rows, E] embedding output; ``mask`` is
        the rectangular (mbias, kvinfo) pair or a PackedBatch.  With ``last_rows`` (LastLayerRows) the
        last layer runs on those rows only and the result is [B*Sq, hidden]."""
        c, f = self.config, self.flat
        m = "albert.encoder.embedding_hidden_mapping_in."
        h = ops.linear(x, f.w(m + "weight"), f.w(m + "bias"), f.g(m + "weight"), f.g(m + "bias"))
        views = [[self._layer_views(g, i) for i in range(c.inner_group_num)] for g in range(c.num_hidden_groups)]
        if _DGRAD_WT and torch.is_grad_enabled():
            views = [[_with_transposed_weights(lv) for lv in row] for row in views]
        per_group = c.num_hidden_layers // c.num_hidden_groups
        group_of = [int(layer / per_group) for layer in range(c.num_hidden_layers)]
        pruned = c.num_hidden_layers - 1 if last_rows is not None else None
        # The applications of each group's weights that share one slab series.  The compact layer
        # accumulates its weight gradients directly, outside the series: the application before it
        # opens the series.
        uses = [[layer for layer in range(c.num_hidden_layers) if group_of[layer] == g and layer != pruned]
                for g in range(c.num_hidden_groups)]
        for layer in range(c.num_hidden_layers):
            g = group_of[layer]
            for i in range(c.inner_group_num):
                lv = views[g][i]
                if layer != pruned and _SHARED_WGRAD and torch.is_grad_enabled():
                    # backward runs the layers in reverse: the last application is the first to
                    # write the weight's gradient slabs, the first application sums them in
                    lv = dict(lv, wg_first=layer == uses[g][-1], wg_last=layer == uses[g][0])
                h = self._albert_layer(h, lv, mask, Sp, last_rows if layer == pruned else None)
        return h

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self._p.values())


class AlbertForPreTraining(AlbertPreTrainedModel):
    """HF ``AlbertForPreTraining`` (MLM head with the decoder tied to the word embeddings + SOP head)."""

    def _add_heads(self):
        c = self.config
        E, H, V = c.embedding_size, c.hidden_size, c.vocab_size
        add = self._add
        add("predictions.bias", V, init="zeros")
        add("predictions.dense.weight", E, H)
        add("predictions.dense.bias", E, init="zeros")
        add("predictions.LayerNorm.weight", E, init="ones")
        add("predictions.LayerNorm.bias", E, init="zeros")
        add("sop_classifier.classifier.weight", 2, H)
        add("sop_classifier.classifier.bias", 2, init="zeros")

    def hf_state_dict(self) -> Dict[str, torch.Tensor]:
        """state dict with exactly HF AlbertForPreTraining's keys (tied decoder included)."""
        sd = super().hf_state_dict()
        sd["predictions.decoder.weight"] = sd["albert.embeddings.word_embeddings.weight"]
        sd["predictions.decoder.bias"] = sd["predictions.bias"]
        return sd

    def _trunk(self, input_ids, attention_mask, token_type_ids, labels, mlm_positions, mlm_labels, pack_sequences,
               lengths):
        """Encoder pass of ``forward`` / ``evaluate_batch``: (h, S', PackedBatch or None, row0, sel),
        row0[b] the row of sequence b's first token in h.  With sel (a LastLayerRows) h is the last
        layer's compact output, S' its slot length."""
        pk = self._packed(pack_sequences, input_ids, attention_mask, token_type_ids, lengths,
                          labels if mlm_positions is None else None)
        if pk is not None:
            h, _ = self.encode(packed=pk)
            return h, None, pk, pk.row_start, None  # (b, position) -> row0[b] + position
        sel = self._last_rows(input_ids, labels, mlm_positions, mlm_labels)
        if sel is not None:
            # h holds the compact rows: sequence b's [CLS] row at b * Sq, its MLM rows behind it
            h, _ = self.encode(input_ids, attention_mask, token_type_ids, last_rows=sel)
            return h, sel.Sq, None, torch.arange(input_ids.shape[0], device=h.device) * sel.Sq, sel
        h, Sp = self.encode(input_ids, attention_mask, token_type_ids)
        return h, Sp, None, torch.arange(input_ids.shape[0], device=h.device) * Sp, None

    def _last_rows(self, input_ids, labels, mlm_positions, mlm_labels):
        """The compact-row plan of this call's last layer, or None when the full layer runs (no MLM
        targets, an unsupported head size, the switch off, or nothing to save)."""
        if not self.last_layer_rows_supported():
            return None
        Sp = (input_ids.shape[1] + 63) // 64 * 64
        if mlm_positions is not None:
            return LastLayerRows.from_positions(mlm_positions, mlm_labels, Sp)
        if labels is not None:
            return LastLayerRows.from_labels(labels, Sp)
        return None

    @staticmethod
    def _mlm_targets(pk, row0, S, Sp, labels, mlm_positions, mlm_labels, sel=None):
        """(rows of h under the MLM head, their targets), or (None, None) without MLM targets."""
        if sel is not None:  # h is the compact output of the last layer
            return sel.head_rows, sel.targets
        if mlm_positions is None and labels is not None:
            if pk is not None:  # packed labels keep the (b, position) order of the rectangular ones
                flat_lab = pk.extras["labels"]
                rows = torch.nonzero(flat_lab != -100).squeeze(1)
                return rows, flat_lab[rows]
            flat_lab = labels.reshape(-1)
            pos = torch.nonzero(flat_lab != -100).squeeze(1)
            b_idx, s_idx = pos // S, pos % S
            return b_idx * Sp + s_idx, flat_lab[pos]
        if mlm_positions is not None:
            return (row0[:, None] + mlm_positions).reshape(-1), mlm_labels.reshape(-1)
        return None, None

    def _mlm_logits(self, h, rows):
        c, f = self.config, self.flat
        hm = h.index_select(0, rows)
        p = "predictions."
        t = ops.linear(hm, f.w(p + "dense.weight"), f.w(p + "dense.bias"), f.g(p + "dense.weight"),
                       f.g(p + "dense.bias"))
        t = ops.gelu_new(t)
        t = ops.add_layernorm(t, None, f.p(p + "LayerNorm.weight"), f.p(p + "LayerNorm.bias"),
                              f.g(p + "LayerNorm.weight"), f.g(p + "LayerNorm.bias"), c.layer_norm_eps)
        wname = "albert.embeddings.word_embeddings.weight"
        return ops.linear(t, f.w(wname), f.w(p + "bias"), f.g(wname), f.g(p + "bias"))

    def _sop_logits(self, h, B, Sp, pk, row0):
        c, f = self.config, self.flat
        cls = h.index_select(0, row0) if pk is not None else h.view(B, Sp, -1)[:, 0].contiguous()
        pooled = ops.tanh(ops.linear(cls, f.w("albert.pooler.weight"), f.w("albert.pooler.bias"),
                                     f.g("albert.pooler.weight"), f.g("albert.pooler.bias")))
        if self.training and c.classifier_dropout_prob > 0:
            pooled = F.dropout(pooled, c.classifier_dropout_prob, True)
        s = "sop_classifier.classifier."
        return ops.linear(pooled, f.w(s + "weight"), f.w(s + "bias"), f.g(s + "weight"), f.g(s + "bias"))

    def evaluate_batch(self, batch, lengths=None):
        """Held-out statistics of one batch (a stream's ``next_batch()`` dict), forward only: eval mode
        and ``no_grad`` (the previous mode is restored), the encoder and head path of ``forward``
        (``pack_sequences`` and both MLM target forms included) ending in ``ops.eval_cross_entropy``.
        No gradient buffer is written, no [M, V] gradient is made and no random generator is drawn
        from.  Returns device scalars: ``mlm_loss_sum``, ``mlm_count``, ``mlm_top1``, ``mlm_top5``,
        ``sop_loss_sum``, ``sop_count``, ``sop_correct`` (sums and counts, so batches add up)."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                ids = batch["input_ids"]
                B, S = ids.shape
                labels, pos = batch.get("labels"), batch.get("mlm_positions")
                h, Sp, pk, row0, sel = self._trunk(ids, batch.get("attention_mask"), batch.get("token_type_ids"),
                                                   labels, pos, batch.get("mlm_labels"), None, lengths)
                rows, tgt = self._mlm_targets(pk, row0, S, Sp, labels, pos, batch.get("mlm_labels"), sel)
                if rows is None:
                    raise ValueError("evaluate_batch needs MLM targets: labels or mlm_positions/mlm_labels")
                mlm = ops.eval_cross_entropy(self._mlm_logits(h, rows), tgt, topk=(1, 5))
                sop = ops.eval_cross_entropy(self._sop_logits(h, B, Sp, pk, row0), batch["sentence_order_label"],
                                             topk=(1,))
        finally:
            self.train(was_training)
        return {"mlm_loss_sum": mlm["loss_sum"], "mlm_count": mlm["count"], "mlm_top1": mlm["top1"],
                "mlm_top5": mlm["top5"], "sop_loss_sum": sop["loss_sum"], "sop_count": sop["count"],
                "sop_correct": sop["top1"]}

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, sentence_order_label=None,
                mlm_positions=None, mlm_labels=None, return_logits=False, pack_sequences=None, lengths=None):
        """HF-compatible pre-training forward.

        MLM targets either as HF ``labels`` [B, S] (-100 = ignore) or as fixed-shape
        ``mlm_positions``/``mlm_labels`` [B, P] (BERT's max_predictions_per_seq form; -100 pads) —
        the fixed form needs no host synchronisation and is graph-capturable.

        ``pack_sequences`` (default: the model's attribute) runs the same computation on the packed,
        padding-free token buffer; ``lengths`` are the rows' host-side lengths (without them one
        device synchronisation reads them from ``attention_mask``).  Inputs and ``out`` are unchanged.
        """
        B, S = input_ids.shape
        h, Sp, pk, row0, sel = self._trunk(input_ids, attention_mask, token_type_ids, labels, mlm_positions, mlm_labels,
                                           pack_sequences, lengths)
        out = {}
        # ---- MLM head on masked positions only
        rows, tgt = self._mlm_targets(pk, row0, S, Sp, labels, mlm_positions, mlm_labels, sel)
        loss = None
        if rows is not None:
            logits = self._mlm_logits(h, rows)
            mlm_loss = ops.cross_entropy(logits, tgt)
            out["mlm_loss"] = mlm_loss
            loss = mlm_loss
            if return_logits:
                out["prediction_logits_masked"] = logits
        # ---- SOP head on [CLS]
        sop_logits = self._sop_logits(h, B, Sp, pk, row0)
        out["sop_logits"] = sop_logits
        if sentence_order_label is not None:
            sop_loss = ops.cross_entropy(sop_logits, sentence_order_label)
            out["sop_loss"] = sop_loss
            loss = sop_loss if loss is None else loss + sop_loss
        out["loss"] = loss
        return out


class AlbertForSequenceClassification(AlbertPreTrainedModel):
    """HF ``AlbertForSequenceClassification``: pooler(tanh) on [CLS] -> dropout -> classifier.
    Cross-entropy for ``num_labels > 1``, MSE for regression (``num_labels == 1``).  Used by the
    sahajBERT NCC fine-tuning recipe (reference sahajbert/train_ncc.py)."""

    def __init__(self, config: AlbertConfig, num_labels: Optional[int] = None):
        self.num_labels = int(num_labels or config.num_labels or 2)
        config.num_labels = self.num_labels
        super().__init__(config)

    def _add_heads(self):
        self._add("classifier.weight", self.num_labels, self.config.hidden_size)
        self._add("classifier.bias", self.num_labels, init="zeros")

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, pack_sequences=None,
                lengths=None):
        c, f = self.config, self.flat
        B = input_ids.shape[0]
        pk = self._packed(pack_sequences, input_ids, attention_mask, token_type_ids, lengths)
        if pk is not None:
            h, _ = self.encode(packed=pk)
            cls = h.index_select(0, pk.row_start)
        else:
            h, Sp = self.encode(input_ids, attention_mask, token_type_ids)
            cls = h.view(B, Sp, -1)[:, 0].contiguous()
        pooled = ops.tanh(ops.linear(cls, f.w("albert.pooler.weight"), f.w("albert.pooler.bias"),
                                     f.g("albert.pooler.weight"), f.g("albert.pooler.bias")))
        if self.training and c.classifier_dropout_prob > 0:
            pooled = F.dropout(pooled, c.classifier_dropout_prob, True)
        logits = ops.linear(pooled, f.w("classifier.weight"), f.w("classifier.bias"), f.g("classifier.weight"),
                            f.g("classifier.bias"))
        out = {"logits": logits}
        if labels is not None:
            if self.num_labels == 1:
                out["loss"] = F.mse_loss(logits.float().view(-1), labels.float().view(-1))
            else:
                out["loss"] = ops.cross_entropy(logits, labels)
        return out


class AlbertForTokenClassification(AlbertPreTrainedModel):
    """HF ``AlbertForTokenClassification`` (no pooler): dropout -> per-token classifier, CE over the
    positions whose label != -100.  Used by the sahajBERT NER recipe (reference sahajbert/train_ner.py)."""

    add_pooler = False

    def __init__(self, config: AlbertConfig, num_labels: Optional[int] = None):
        self.num_labels = int(num_labels or config.num_labels or 2)
        config.num_labels = self.num_labels
        super().__init__(config)

    def _add_heads(self):
        self._add("classifier.weight", self.num_labels, self.config.hidden_size)
        self._add("classifier.bias", self.num_labels, init="zeros")

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, pack_sequences=None,
                lengths=None):
        c, f = self.config, self.flat
        B, S = input_ids.shape
        pk = self._packed(pack_sequences, input_ids, attention_mask, token_type_ids, lengths, labels)
        if pk is not None:
            h, _ = self.encode(packed=pk)
        else:
            h, Sp = self.encode(input_ids, attention_mask, token_type_ids)
        if self.training and c.classifier_dropout_prob > 0:
            h = F.dropout(h, c.classifier_dropout_prob, True)
        logits = ops.linear(h, f.w("classifier.weight"), f.w("classifier.bias"), f.g("classifier.weight"),
                            f.g("classifier.bias"))
        if pk is not None:
            # logits come back unpacked as [B, S, labels] (rows of padded positions past a sequence's
            # slot do not exist: zeros); the loss runs on the packed rows, whose filler carries -100
            out = {"logits": unpack_rows(logits, pk, S)}
            if labels is not None:
                out["loss"] = ops.cross_entropy(logits, pk.extras["labels"])
            return out
        out = {"logits": logits.view(B, Sp, -1)[:, :S]}
        if labels is not None:
            lab = labels
            if Sp != S:
                lab = F.pad(labels, (0, Sp - S), value=-100)
            out["loss"] = ops.cross_entropy(logits, lab.reshape(-1))
        return out


def flops_per_sample(config: AlbertConfig, seq_len: int, masked_per_seq: int) -> float:
    """Model FLOPs (fwd+bwd = 3x fwd) per training sample, used for MFU reporting."""
    c = config
    H, I, E = c.hidden_size, c.intermediate_size, c.embedding_size
    per_tok_layer = 2 * (4 * H * H + 2 * H * I)
    attn = 2 * 2 * seq_len * H
    fwd = seq_len * (c.num_hidden_layers * (per_tok_layer + attn) + 2 * E * H)
    fwd += masked_per_seq * (2 * H * E + 2 * E * c.vocab_size)
    return 3.0 * fwd
