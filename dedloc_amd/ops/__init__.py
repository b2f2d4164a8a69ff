"""Differentiable building blocks over the ``dedloc::`` operators.

Parameter gradients are *accumulated as a side effect* straight into fp32 views of the flat
gradient buffer (``g*`` arguments), Megatron-style "gradient accumulation fusion": autograd only
carries activation gradients, and ALBERT's shared layer simply accumulates its 24 weight-gradient
contributions into the same fp32 view.  Weights are consumed as bf16 views of the flat bf16
parameter copy that the optimizer refreshes after each global step.

Reference parity: these implement the HF ``AlbertForPreTraining`` forward used by
``albert/run_trainer.py:56-70`` — Linear, gelu_new, LayerNorm(eps 1e-12),
scaled-dot-product attention with key padding mask, tanh pooler, cross-entropy.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import load_native, native_loaded  # noqa: F401

OPS = torch.ops.dedloc


def _needs_grad(*xs):
    return any(isinstance(x, torch.Tensor) and x.requires_grad for x in xs)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, gw, gb, epilogue):
        ctx.save_for_backward(x, w)
        ctx.gw, ctx.gb = gw, gb
        return OPS.gemm(x, w, b, None, False, True, epilogue)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = OPS.gemm(dy, w, None, None, False, False, 0)
        if ctx.gw is not None:
            OPS.gemm_acc_f32(dy, x, ctx.gw, True, False)
        if ctx.gb is not None:
            OPS.bias_grad(dy, ctx.gb, True)
        return dx, None, None, None, None, None


def linear(x, w, b=None, gw=None, gb=None):
    """y = x @ w.T + b with fp32 gradient accumulation into gw / gb.  x: [M, K] bf16, w: [N, K]."""
    return _Linear.apply(x, w, b, gw, gb, 0)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return OPS.gelu_fwd(h)

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        return OPS.gelu_bwd(dy.contiguous(), h)


def gelu_new(h):
    return _Gelu.apply(h)


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = OPS.tanh_fwd(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return OPS.tanh_bwd(dy.contiguous(), y)


def tanh(x):
    return _Tanh.apply(x)


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, ggamma, gbeta, eps):
        y, s, mean, rstd = OPS.layernorm_fwd(x, res, gamma, beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        ctx.ggamma, ctx.gbeta, ctx.has_res = ggamma, gbeta, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        s, gamma, mean, rstd = ctx.saved_tensors
        gg, gb = ctx.ggamma, ctx.gbeta
        if gg is None:
            gg = torch.zeros_like(gamma)
            gb = torch.zeros_like(gamma)
        ds = OPS.layernorm_bwd(dy.contiguous(), s, gamma, mean, rstd, gg, gb, True)
        return ds, (ds if ctx.has_res else None), None, None, None, None, None


def add_layernorm(x, res, gamma, beta, ggamma=None, gbeta=None, eps=1e-12):
    """LayerNorm(x + res) (res may be None); gamma/beta are fp32, grads accumulate into ggamma/gbeta."""
    return _AddLayerNorm.apply(x, res, gamma, beta, ggamma, gbeta, eps)


_LOG2E = math.log2(math.e)


def _bmm_f32(a, b):
    """[N, M, K] x [N, K, P] bf16 -> fp32 without rounding the product through bf16 (the own
    batched GEMM kernel; transposed operands are read in place)."""
    return OPS.bmm(a, b, True)


def _bmm(a, b):
    """[N, M, K] x [N, K, P] bf16 -> bf16 on the own batched GEMM kernel."""
    return OPS.bmm(a, b, False)


def _attn_split(qkv, H, S):
    T, ld = qkv.shape
    D = ld // (3 * H)
    B = T // S
    x = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4)  # 3, B, H, S, D
    return (x[0].reshape(B * H, S, D), x[1].reshape(B * H, S, D), x[2].reshape(B * H, S, D)), B, D


def attn_composed_fwd(qkv, mbias, H, S, scale):
    """Attention for head sizes outside ``FUSED_HEAD_DIMS``: batched bf16
    GEMMs with fp32 scores around the ``attn_softmax_fwd`` kernel (scale, key bias, log2-unit
    softmax in one pass) — same inputs / outputs as ``attn_fwd`` (out [B*S, H*D] bf16, lse
    [B, H, S] fp32 in log2 units), but the [B*H, S, S] scores go through HBM."""
    (q, k, v), B, D = _attn_split(qkv, H, S)
    s = _bmm_f32(q, k.transpose(1, 2))
    p, lse = OPS.attn_softmax_fwd(s, mbias, H, scale * _LOG2E)
    del s
    o = _bmm(p, v)
    return o.view(B, H, S, D).transpose(1, 2).reshape(B * S, H * D), lse.view(B, H, S)


def attn_composed_bwd(qkv, mbias, out, dout, lse, H, S, scale, dbias=None):
    """Backward of ``attn_composed_fwd`` (probabilities recomputed from lse by the
    ``attn_softmax_bwd`` kernel, which also forms dS); dQKV in the packed layout, and — like the
    fused backward — the QKV bias gradient accumulated into ``dbias``."""
    (q, k, v), B, D = _attn_split(qkv, H, S)
    do = dout.view(B, S, H, D).transpose(1, 2).reshape(B * H, S, D)
    o = out.view(B, S, H, D).transpose(1, 2).reshape(B * H, S, D)
    s = _bmm_f32(q, k.transpose(1, 2))
    dp = _bmm_f32(do, v.transpose(1, 2))
    delta = (do.float() * o.float()).sum(-1)
    p, ds = OPS.attn_softmax_bwd(s, dp, mbias, lse.reshape(-1).contiguous(), delta.reshape(-1), H,
                                 scale * _LOG2E, scale)
    del s, dp
    dv = _bmm(p.transpose(1, 2), do)
    dq = _bmm(ds, k)
    dk = _bmm(ds.transpose(1, 2), q)
    g = torch.stack([dq, dk, dv], 0).view(3, B, H, S, D).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * H * D)
    if dbias is not None:  # query: colsum dQ; key: 0 (softmax shift invariance); value: colsum dout
        HD = H * D
        dbias[:HD] += g[:, :HD].float().sum(0)
        dbias[2 * HD:] += dout.float().sum(0)
    return g


# Head sizes the fused flash kernels serve on the GPU; every other size takes the composed path.
# Benchmarks and tests narrow this tuple (``ops.FUSED_HEAD_DIMS = (64,)``) to run the composed path
# at head_dim 128.
FUSED_HEAD_DIMS = (64, 128)


def _fused_attention(qkv, H):
    return not qkv.is_cuda or qkv.shape[-1] // (3 * H) in FUSED_HEAD_DIMS


def attn_fwd(qkv, mbias, H, S, scale, kvinfo=None):
    """The fused flash kernels for the head sizes in ``FUSED_HEAD_DIMS`` (CPU: the fp32 reference),
    else the composed path."""
    if _fused_attention(qkv, H):
        return OPS.attn_fwd(qkv, mbias, H, S, scale, kvinfo)
    return attn_composed_fwd(qkv, mbias, H, S, scale)


def attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo=None, dbias=None):
    if _fused_attention(qkv, H):
        return OPS.attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo, dbias)
    return attn_composed_bwd(qkv, mbias, out, dout, lse, H, S, scale, dbias)


def attn_fwd_q(q, kv, qcnt, mbias, H, S, scale, kvinfo=None):
    """Fused attention of compact queries: ``q`` [B*Sq, H*64] holds sequence b's queries in the
    first ``qcnt[b]`` rows of its slot of ``Sq`` rows (a multiple of 64, at most S); keys and values
    are all rows of ``kv`` [B*S, 2*H*64] (K | V; a column slice of the fused QKV buffer will do).
    Returns out [B*Sq, H*64] and lse [B, H, Sq]; slot rows past ``qcnt[b]`` are dead (zeros in out,
    nothing written to lse).  Each
    live row equals the same row of ``attn_fwd`` bit for bit.  Head_dim 64 only: there is no
    head_dim-128, composed or packed form."""
    return OPS.attn_fwd_q(q, kv, qcnt, mbias, H, S, scale, kvinfo)


def attn_bwd_q(q, kv, qcnt, mbias, out, dout, lse, H, S, scale, kvinfo=None, dbias=None):
    """Backward of ``attn_fwd_q``: (dq [B*Sq, H*64], dkv [B*S, 2*H*64] over all keys, delta
    [B, H, Sq]); the fused bias gradient in ``dbias`` (fp32 [3*H*64]) counts live rows only."""
    return OPS.attn_bwd_q(q, kv, qcnt, mbias, out, dout, lse, H, S, scale, kvinfo, dbias)


def attn_varlen_fwd(qkv, packed, H, scale):
    """Fused attention over a packed variable-length batch (``data.packing.PackedBatch``): out
    [T, H*D] bf16, lse [H, T] fp32 (log2 units).  Only the head sizes in ``FUSED_HEAD_DIMS``: there
    is no composed path for packed batches, any other head size is an error."""
    D = qkv.shape[-1] // (3 * H)
    if D not in FUSED_HEAD_DIMS:
        raise RuntimeError(f"dedloc_amd: packed batches need a fused attention head size {FUSED_HEAD_DIMS}, "
                           f"got head_dim {D}")
    return OPS.attn_varlen_fwd(qkv, packed.seqinfo, packed.seqinfo_host, H, scale)


def attn_varlen_bwd(qkv, packed, out, dout, lse, H, scale, dbias=None):
    return OPS.attn_varlen_bwd(qkv, packed.seqinfo, packed.seqinfo_host, out, dout, lse, H, scale, dbias)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, mbias, H, S, scale):
        out, lse = attn_fwd(qkv, mbias, H, S, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.mbias, ctx.H, ctx.S, ctx.scale = mbias, H, S, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        dqkv = attn_bwd(qkv, ctx.mbias, out, dout.contiguous(), lse, ctx.H, ctx.S, ctx.scale)
        return dqkv, None, None, None, None


def attention(qkv, mbias, num_heads, seq_len, scale=None):
    """Fused self-attention over a packed [B*S, 3*H*D] QKV buffer -> [B*S, H*D].

    ``mbias`` is the [B, S] fp32 additive key bias in log2 units (0 = keep, -1e30 = masked).
    """
    d = qkv.shape[-1] // (3 * num_heads)
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    return _Attention.apply(qkv, mbias, num_heads, seq_len, scale)


class _EmbedLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, ids, tt, wemb, pemb, temb, gamma, beta, gw, gp, gt, ggamma, gbeta, S, eps):
        y, s, mean, rstd = OPS.embed_ln_fwd(ids, tt, wemb, pemb, temb, gamma, beta, S, eps)
        ctx.save_for_backward(ids, s, gamma, mean, rstd)
        ctx.tt = tt
        ctx.grads = (gw, gp, gt, ggamma, gbeta)
        ctx.S = S
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, s, gamma, mean, rstd = ctx.saved_tensors
        gw, gp, gt, gg, gb = ctx.grads
        if gw is not None:
            ds = OPS.layernorm_bwd(dy.contiguous(), s, gamma, mean, rstd, gg, gb, True)
            OPS.embed_bwd(ds, ids, ctx.tt, gw, gp, gt, ctx.S)
        return (None,) * 15


class _EmbedLNPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, ids, tt, pos, wemb, pemb, temb, gamma, beta, gw, gp, gt, ggamma, gbeta, eps):
        y, s, mean, rstd = OPS.embed_ln_pos_fwd(ids, tt, pos, wemb, pemb, temb, gamma, beta, eps)
        ctx.save_for_backward(ids, pos, s, gamma, mean, rstd)
        ctx.tt = tt
        ctx.grads = (gw, gp, gt, ggamma, gbeta)
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, pos, s, gamma, mean, rstd = ctx.saved_tensors
        gw, gp, gt, gg, gb = ctx.grads
        if gw is not None:
            ds = OPS.layernorm_bwd(dy.contiguous(), s, gamma, mean, rstd, gg, gb, True)
            OPS.embed_pos_bwd(ds, ids, ctx.tt, pos, gw, gp, gt)
        return (None,) * 15


def embed_layernorm_packed(ids, tt, pos, wemb, pemb, temb, gamma, beta, grads=(None,) * 5, eps=1e-12):
    """``embed_layernorm`` for a packed batch: ids / tt int64[T], pos int32[T] (each row's offset
    inside its slot) -> [T, E] bf16."""
    anchor = torch.empty(0, device=ids.device, requires_grad=True)
    return _EmbedLNPacked.apply(anchor, ids.contiguous(), None if tt is None else tt.contiguous(), pos.contiguous(),
                                wemb, pemb, temb, gamma, beta, *grads, eps)


def embed_layernorm(ids, tt, wemb, pemb, temb, gamma, beta, grads=(None,) * 5, eps=1e-12):
    """ALBERT embeddings: LN(word[ids] + pos[arange(S)] + type[tt]) -> [B*S, E] bf16.

    The fp32 master tables are read directly; gradients are scattered into ``grads`` =
    (g_word, g_pos, g_type, g_ln_gamma, g_ln_beta).
    """
    B, S = ids.shape
    anchor = torch.empty(0, device=ids.device, requires_grad=True)
    return _EmbedLN.apply(anchor, ids.reshape(-1).contiguous(), None if tt is None else tt.reshape(-1).contiguous(),
                          wemb, pemb, temb, gamma, beta, *grads, S, eps)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        loss, dlogits = OPS.xent_fwd_bwd(logits, labels, False, ignore_index)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        # the kernel already produced d(mean loss)/dlogits; scale in place by the upstream grad (a
        # no-op on the device when it is 1, the usual loss.backward() seed: no host sync, no pass)
        if dlogits.dtype == torch.bfloat16 and dlogits.is_contiguous():
            OPS.scale_by_(dlogits, dloss.reshape(1).float())
            return dlogits, None, None
        return dlogits.mul_(dloss.to(dlogits.dtype)), None, None


def cross_entropy(logits, labels, ignore_index=-100):
    """Mean token cross-entropy over rows whose label != ignore_index (fused fwd+bwd kernel)."""
    return _CrossEntropy.apply(logits.contiguous(), labels.reshape(-1).contiguous(), ignore_index)


@torch.no_grad()
def eval_cross_entropy(logits, labels, ignore_index=-100, topk=(1, 5)):
    """Evaluation cross-entropy over rows whose label != ignore_index, forward only (the
    ``xent_eval`` kernel: one read of the logits, no gradient).  Returns device scalars
    ``loss_sum`` (fp64 sum of the per-row losses), ``count`` (int64) and one ``top{k}`` (int64 number
    of rows whose label ranks below k; ties go to the lower index).  The per-row outputs are
    reduced by plain ``sum`` — a fixed order, so two calls agree bitwise — and nothing is read back."""
    if not (logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]):
        logits = logits.contiguous()
    row_loss, row_rank = OPS.xent_eval(logits, labels.reshape(-1).contiguous(), ignore_index)
    valid = row_rank >= 0
    out = {"loss_sum": row_loss.sum(dtype=torch.float64), "count": valid.sum()}
    for k in topk:
        out[f"top{k}"] = (valid & (row_rank < k)).sum()
    return out


@torch.no_grad()
def knn_topk(q, bank, k, splits=0):
    """The ``k`` nearest bank rows of every query row by dot product (the fused similarity + top-k
    kernel: no score matrix in memory): ``vals`` [Q, k] fp32 and ``idx`` [Q, k] int32, ordered by
    (score descending, bank index ascending).  ``q`` [Q, D] and ``bank`` [N, D] are brought to
    contiguous bf16; ``splits`` = 0 lets the kernel choose its number of bank slices."""
    return OPS.knn_topk(q.to(torch.bfloat16).contiguous(), bank.to(torch.bfloat16).contiguous(), int(k), int(splits))


@torch.no_grad()
def knn_classify(q, bank, bank_labels, targets, num_classes, k=200, sigma=0.1, splits=0):
    """Weighted k-nearest-neighbour classification of the rows of ``q`` against a labelled bank
    (``knn_topk`` + ``knn_vote``, k cut to the bank's size).  Returns device scalars ``count`` (rows
    whose target is a class id), ``top1`` and ``top5`` (int64: rank 0, rank 0..4; a target no
    neighbour voted for has rank -1 and is a miss) and the per-row ``pred`` / ``rank`` (int32).
    Nothing is read back."""
    k = max(1, min(int(k), bank.shape[0]))
    vals, idx = knn_topk(q, bank, k, splits)
    targets = targets.to(torch.int64).reshape(-1).contiguous()
    pred, rank = OPS.knn_vote(vals, idx, bank_labels.to(torch.int32).contiguous(), targets, int(num_classes),
                              float(sigma))
    count = ((targets >= 0) & (targets < int(num_classes))).sum()
    return {"count": count, "top1": (rank == 0).sum(), "top5": ((rank >= 0) & (rank < 5)).sum(), "pred": pred,
            "rank": rank}


__all__ = [
    "linear", "gelu_new", "tanh", "add_layernorm", "attention", "embed_layernorm", "cross_entropy",
    "eval_cross_entropy", "knn_topk", "knn_classify", "OPS",
    "load_native", "native_loaded",
]

# The gfx950 library is mandatory wherever a GPU is visible (fails loudly otherwise); on a CPU-only
# host the CPU implementations registered in _lib serve the plumbing configuration.
load_native()
