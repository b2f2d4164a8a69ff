"""Shared checks of the GEMM kernels (tests/test_gemm_checks_cpu.py, tests/test_gemm_exact_gpu.py).

Two kinds of check, both per element (a Frobenius-norm ratio cannot see one wrong 16-byte store):

* exact: operands from a dyadic grid (A, residual: integers; B: integers times 2^-2; bias and the
  fp32 ``c``: integers), small enough that every product and every partial sum, in any order, is
  exact in fp32.  Split counts, atomics order, MFMA-internal order and slab order then cannot change
  the result: a bf16 output must be bit-equal to ONE round-to-nearest-even of the fp64 reference,
  an fp32 output to the reference itself (``expect_exact``).
* bounded: real-valued data against the standard fp32 dot-product bound (``expect_bounded``).

Operands are generated on the host (one generator per seed, the same values in the CPU and the GPU
tier) and moved to the device the caller names."""
import math
from dataclasses import dataclass

import torch

GRID = 0.25          # B's grid: integers times 2^-2, so sums are quarter-integers
B_MAX = 3            # |B| <= 3 grid units
BIAS_MAX = 8
C_MAX = 1000
ROUNDING_FLOOR = 0.10  # share of outputs that must not be representable in bf16 before rounding
TILE = 256           # gemm8.hip / gemm.hip output tile

# ------------------------------------------------------------------------------------------------
# the shapes the GPU tier runs, (M, N, K); the CPU tier checks the generator on every one of them
# ------------------------------------------------------------------------------------------------
M_TAILS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257)
GEMM8_TAIL_SHAPES = tuple((m, 256, 64) for m in M_TAILS)
GEMM8_DEPTH_SHAPES = tuple((256, 256, k) for k in (64, 128, 192, 256, 320))
GEMM8_ORDER_SHAPES = ((1025, 256, 64), (1300, 768, 128), (1537, 768, 64), (1800, 512, 64))
FUSED_SHAPES = ((300, 256, 128), (257, 512, 64), (1025, 256, 192))
FUSED_N384_SHAPES = tuple((300, 384, k) for k in (64, 128))
FUSED_NARROW_SHAPES = ((256, 128, 64),)
# weight gradients: (tokens, rows of c, columns of c, split count wgrad_splits8 gives)
WGRAD_TN = ((64, 256, 256, 1), (512, 256, 256, 2), (1344, 256, 256, 3), (4096, 512, 256, 16),
            (25088, 256, 256, 49))
WGRAD_NT = (256, 256, 128)
SHARED_SHAPE = (256, 256, 2048)  # (rows of c, columns of c, tokens)
TILED_SHAPES = tuple((m, n, k) for n in (384, 640) for m in (256, 300) for k in (64, 192))
SMALL_SHAPES = ((1, 1, 1), (37, 70, 96), (129, 65, 33), (128, 192, 40))
SMALL_SPLIT_SHAPES = ((37, 70, 1100, 2), (200, 128, 2049, 4))  # (M, N, K, slabs)
BMM_SHAPES = ((5, 37, 70, 96), (6, 192, 64, 192))  # (batch, M, N, K)
SPLIT_DEFECT = (256, 256, 66624)  # gemm.hip: 65 splits of 1024 rows used to drop the last 64 rows

# bf16-output shapes whose exact check must see rounding: ROUNDING_FLOOR holds on each of them
BF16_STORE_SHAPES = (GEMM8_TAIL_SHAPES + GEMM8_DEPTH_SHAPES + GEMM8_ORDER_SHAPES + FUSED_SHAPES + FUSED_N384_SHAPES +
                     TILED_SHAPES + tuple(s[:3] for s in SMALL_SPLIT_SHAPES) + ((37, 70, 96),))
# With |A| <= 8 and |B| <= 3 grid units a sum of K products is at most 24 K grid units, and a
# quarter-integer needs rounding only from 257 grid units on; the bias and residual add at most 64.
# Below K = 64 that is out of reach for all but a sliver of the outputs of any distribution inside
# the ranges (K = 1: never), so for these only the exactness precondition is checked.
SHORT_K_SHAPES = ((1, 1, 1), (129, 65, 33), (128, 192, 40))


# ------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, amax):
    return torch.randint(-amax, amax + 1, shape, generator=g)


def _tilted(g, rows, K, amax, pattern):
    """[rows, K] integers in [-amax, amax].  With ``pattern`` (a [K] vector of +-1) the sign of each
    entry agrees with (row sign) * pattern with a per-row probability in [0.75, 1]: the dot products
    of two such operands do not cancel, so they spread over +-24 K grid units and a large share needs
    rounding to bf16 (independent signs give |sum| ~ sqrt(K), all representable at K = 64)."""
    if pattern is None:
        return _ints(g, (rows, K), amax)
    mag = torch.randint(0, amax + 1, (rows, K), generator=g)
    p = 0.75 + 0.25 * torch.rand(rows, 1, generator=g)
    agree = torch.rand(rows, K, generator=g) < p
    rowsign = torch.randint(0, 2, (rows, 1), generator=g) * 2 - 1
    return mag * torch.where(agree, 1, -1) * rowsign * pattern[None, :]


@dataclass
class Exact:
    """One exact problem out = a @ b^T (+ bias) (+ res) (+ c): a [M, K] and res [M, N] bf16, b [N, K]
    bf16, bias [N] fp32, c [M, N] fp32 (each None when absent)."""
    a: torch.Tensor
    b: torch.Tensor
    bias: torch.Tensor = None
    res: torch.Tensor = None
    c: torch.Tensor = None

    @property
    def shape(self):
        return self.a.shape[0], self.b.shape[0], self.a.shape[1]

    def ref64(self):
        r = torch.matmul(self.a.double(), self.b.double().t())
        if self.bias is not None:
            r = r + self.bias.double()
        if self.res is not None:
            r = r + self.res.double()
        if self.c is not None:
            r = r + self.c.double()
        return r

    def abs_ab(self):
        return torch.matmul(self.a.double().abs(), self.b.double().abs().t())

    def extras(self):
        """|bias| + |R| + |c| per output element (fp64; a scalar 0 when none is present)."""
        e = 0.0
        if self.bias is not None:
            e = e + self.bias.double().abs()
        if self.res is not None:
            e = e + self.res.double().abs()
        if self.c is not None:
            e = e + self.c.double().abs()
        return e


def check_exactness_precondition(p, grid=GRID):
    """max|A| max|B| K + |bias| + |R| + |c| < 2^24 in grid units: every partial sum of the products,
    the epilogue operands included, is an integer number of grid units below 2^24, hence exact in fp32."""
    M, N, K = p.shape
    a, b = p.a.double(), p.b.double() / grid
    assert bool((a == a.round()).all()) and bool((b == b.round()).all()), "operands off the dyadic grid"
    total = float(a.abs().max()) * float(b.abs().max()) * K
    for t in (p.bias, p.res, p.c):
        if t is not None:
            t = t.double()
            assert bool((t == t.round()).all()), "epilogue operand off the integer grid"
            total += float(t.abs().max()) / grid
    assert total < 2.0 ** 24, f"exactness precondition violated: {total} grid units at {p.shape}"
    return total


def exact_problem(M, N, K, *, seed=0, a_max=8, b_max=B_MAX, grid=GRID, bias=False, residual=False, c=False,
                  tilt=True, device="cpu"):
    g = _gen(seed * 1000003 + M * 10007 + N * 101 + K)
    pattern = torch.randint(0, 2, (K,), generator=g) * 2 - 1 if tilt else None
    a = _tilted(g, M, K, a_max, pattern).to(torch.bfloat16)
    b = (_tilted(g, N, K, b_max, pattern).double() * grid).to(torch.bfloat16)
    p = Exact(a, b)
    if bias:
        p.bias = _ints(g, (N,), BIAS_MAX).float()
    if residual:
        p.res = _ints(g, (M, N), a_max).to(torch.bfloat16)
    if c:
        p.c = _ints(g, (M, N), C_MAX).float()
    check_exactness_precondition(p, grid)
    dev = torch.device(device)
    for f in ("a", "b", "bias", "res", "c"):
        t = getattr(p, f)
        if t is not None:
            setattr(p, f, t.to(dev))
    return p


def grid_values(shape, amax, seed, *, grid=GRID, dtype=torch.bfloat16, device="cpu"):
    """Integers in [-amax, amax] times ``grid`` (an activation-like operand such as gemm_dgelu's
    pre-activation F or gemm_dmul's stored derivative D)."""
    return (_ints(_gen(seed), shape, amax).double() * grid).to(dtype).to(device)


def needs_rounding_share(ref64):
    """Share of the reference values that bf16 cannot represent (they test the rounding, ties included)."""
    return float((ref64.float().bfloat16().double() != ref64).double().mean())


def check_rounding_floor(ref64, what=""):
    share = needs_rounding_share(ref64)
    assert share >= ROUNDING_FLOOR, f"{what}: only {share:.1%} of the outputs need rounding to bf16"
    return share


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def expect_exact(got, ref64, what="", tile=None):
    """``got`` (bf16: one round-to-nearest-even of ``ref64``; fp32: ``ref64`` itself) bit for bit."""
    assert got.dtype in (torch.bfloat16, torch.float32), got.dtype
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    want = ref64.float().to(got.dtype)
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.reshape(-1, bad.shape[-1]).nonzero()[:6].tolist() if bad.dim() >= 2 else bad.nonzero()[:6].tolist()
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    shown = [(r, c, float(g2[r, c]), float(w2[r, c])) for r, c in idx] if bad.dim() >= 2 else \
        [(i[0], float(got[i[0]]), float(want[i[0]])) for i in idx]
    msg = f"{what}: {n} of {bad.numel()} elements differ; first (row, col, got, want): {shown}"
    if tile and bad.dim() >= 2:
        r, c = idx[0]
        msg += f"; first in tile row {r // tile}, tile column {c // tile}, in-tile row {r % tile}, in-tile column {c % tile}"
    raise AssertionError(msg)


def expect_bounded(got, ref64, absAB, K, out_bf16, extras=0.0, what="", kernel=None):
    """Per element |got - ref| <= (out_bf16 ? 2^-8 |ref| : 0) + 2 K 2^-24 absAB + 2^-24 extras, where
    absAB = |A| |B|^T and extras = |bias| + |R| + |c|.  K u |A||B| bounds an fp32 dot product in any
    summation order; the factor 2 covers the epilogue adds and an MFMA-internal add that is not
    IEEE-sequential; 2^-8 is bf16's half ulp.  Records the worst err / bound; returns it."""
    err = (got.double() - ref64).abs()
    bound = 2.0 * K * 2.0 ** -24 * absAB + 2.0 ** -24 * extras
    if out_bf16:
        bound = bound + 2.0 ** -8 * ref64.abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    worst = float(ratio.max())
    try:
        from conftest import record_margin

        record_margin(f"gemm_elementwise[{what}]", kernel=kernel, K=K, out_bf16=bool(out_bf16), worst_err_over_bound=worst,
                      max_abs_err=float(err.max()), bound=1.0)
    except ImportError:
        pass
    if worst > 1.0:
        flat = int(ratio.reshape(-1).argmax())
        r, c = flat // ratio.shape[-1], flat % ratio.shape[-1]
        raise AssertionError(f"{what}: err / bound = {worst:.3f} at ({r}, {c}); {int((ratio > 1).sum())} elements above 1")
    return worst


def expect_ulp(got, ref64, what=""):
    """A bf16 value of a smooth function: the correctly rounded value or its neighbour —
    |got - ref| <= 2^-7 |ref| + 2^-20 (one bf16 ulp of the reference; 8 fp32 epsilons of
    intermediates <= 2 for a zero crossing)."""
    err = (got.double() - ref64).abs()
    bound = 2.0 ** -7 * ref64.abs() + 2.0 ** -20
    bad = err > bound
    if bool(bad.any()):
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements off by more than one bf16 ulp; first ({r}, {c}): got "
                             f"{float(got[r, c])}, want {float(ref64[r, c])}")


def expect_colsum(dbias, before, C, what=""):
    """dbias (fp32, accumulated onto ``before``) against the fp64 column sum of the STORED C, within
    M 2^-24 sum_m |C[m, n]| per column."""
    M = C.shape[0]
    want = before.double() + C.double().sum(0)
    bound = M * 2.0 ** -24 * C.double().abs().sum(0)
    bad = (dbias.double() - want).abs() > bound
    if bool(bad.any()):
        n = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} column sums off; first column {n}: got {float(dbias[n])}, want "
                             f"{float(want[n])} +- {float(bound[n])}")


K0, K1 = 0.7978845608028654, 0.044715


def gelu_new64(h):
    h = h.double()
    return 0.5 * h * (1.0 + torch.tanh(K0 * (h + K1 * h ** 3)))


def gelu_new_grad64(h):
    h = h.double()
    t = torch.tanh(K0 * (h + K1 * h ** 3))
    return 0.5 * (1.0 + t) + 0.5 * h * (1.0 - t * t) * K0 * (1.0 + 3.0 * K1 * h * h)


def rel(a, b):
    """The whole-tensor metric of the older GEMM tests (kept to show what it cannot see)."""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------
# planted corruptions (tests/test_gemm_checks_cpu.py): each returns a damaged copy of a correct output
# ------------------------------------------------------------------------------------------------
def flip_one_ulp(out, r, c):
    bad = out.clone()
    bits = bad.view(torch.int16)
    bits[r, c] += 1
    return bad


def zero_chunk(out, r, c8):
    bad = out.clone()
    bad[r, c8 * 8:c8 * 8 + 8] = 0
    return bad


def duplicate_last_row(out):
    bad = out.clone()
    bad[-1] = bad[-2]
    return bad


def shift_bias_block(p, block):
    """The correct bf16 output of ``p`` except that the 32 columns of ``block`` took the bias of the
    column to their left."""
    ref = p.ref64()
    cols = slice(block * 32, block * 32 + 32)
    bias = p.bias.double()
    ref[:, cols] += (torch.roll(bias, 1)[cols] - bias[cols])
    return ref.float().bfloat16()


# ------------------------------------------------------------------------------------------------
# backend counters (dedloc_ws::gemm_backend_counts): which kernel took a call
# ------------------------------------------------------------------------------------------------
BACKENDS = ("gemm8", "gemm", "gemm_small")


def backend_counts():
    return tuple(int(v) for v in torch.ops.dedloc_ws.gemm_backend_counts())


class took:
    """``with took(gemm8=1): op(...)``: the launches inside the block, per kernel, must be exactly these."""

    def __init__(self, what="", **want):
        assert set(want) <= set(BACKENDS), want
        self.want = tuple(want.get(k, 0) for k in BACKENDS)
        self.what = what

    def __enter__(self):
        self.before = backend_counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            got = tuple(b - a for a, b in zip(self.before, backend_counts()))
            assert got == self.want, (f"{self.what}: launches per kernel {dict(zip(BACKENDS, got))}, expected "
                                      f"{dict(zip(BACKENDS, self.want))}")
        return False
