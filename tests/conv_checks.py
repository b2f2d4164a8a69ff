"""Shared checks of the convolution kernels (tests/test_conv_checks_cpu.py, tests/test_conv_exact_gpu.py).

A convolution is linear, so the two per-element checks of tests/gemm_checks.py carry over:

* exact: images and upstream gradients are small integers, weights integers times 2^-2, BN operands
  half-integers and powers of two, small enough that every product and every partial sum, in any
  order, is exact in fp32.  Tile order, MFMA-internal order, split count and atomics order then cannot
  change a result: a bf16 output must be bit-equal to ONE round-to-nearest-even of the fp64 reference,
  an fp32 weight gradient to the reference itself (``expect_exact_conv`` / ``expect_exact_wgrad``).
  Patches overlap, so an image cannot carry a per-k sign pattern; instead images and data-gradient
  inputs are non-negative and the weights of each channel the sum does not run over (the output
  channel; for a data gradient the input channel) lean to one sign (agreement probability 0.75-1),
  which spreads the sums far enough for most of them to need rounding.
* bounded: real-valued data against gemm_checks.expect_bounded with K = R S C and
  absAB = conv(|x|, |w|).

References are fp64 ``F.unfold`` / ``F.fold`` plus one matmul (a plain matmul for a pointwise conv) on
the operands' device; the CPU tier checks them against ``F.conv2d`` in double.  Operands are generated
on the host (one generator per shape and seed, the same values in both tiers).

A shape is (N, Cin, H, W, Cout, k, stride, pad)."""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import gemm_checks as gc

CL = torch.channels_last
GRID = gc.GRID       # the weights' grid: integers times 2^-2
X_MAX = 16           # images and data-gradient inputs: integers in [0, 16]
W_MAX = gc.B_MAX     # |w| <= 3 grid units
DY_MAX = 8           # weight-gradient inputs: integers in [-8, 8]
PRE_MAX = 8          # pre-filled accumulators (dw, sums): integers in [-8, 8]

# ------------------------------------------------------------------------------------------------
# the shapes the GPU tier runs; the CPU tier checks the generator on every one of them
# ------------------------------------------------------------------------------------------------
FWD_ROW_TAILS = tuple((1, 64, 1, m, 128, 1, 1, 0) for m in (1, 127, 128, 129, 255, 256, 257)) + \
    tuple((1, 64, 1, m, 64, 1, 1, 0) for m in (1, 255, 256, 257, 511, 513))
FWD_CHANNEL_TAILS = tuple((1, 64, 5, 9, k, 3, 1, 1) for k in (8, 64, 72, 128, 136, 192, 200))
FWD_DEPTH = tuple((1, c, 3, 50, 128, 1, 1, 0) for c in (64, 128, 192, 256, 320))  # nk = 1..5, two row tiles
FWD_BORDERS = (
    (2, 64, 1, 1, 64, 3, 1, 1), (2, 64, 1, 2, 64, 3, 1, 1), (2, 64, 2, 3, 64, 3, 1, 1), (2, 64, 3, 3, 64, 3, 1, 1),
    (2, 64, 5, 7, 64, 3, 1, 0),      # no padding
    (2, 64, 4, 6, 128, 3, 1, 2),     # pad wider than the tap reach
    (1, 64, 9, 12, 128, 7, 2, 3),
    (2, 64, 6, 9, 64, 3, 2, 1), (2, 64, 7, 10, 128, 3, 2, 1),
    (2, 64, 7, 9, 64, 1, 2, 0),      # three of four parity classes have no tap
    (2, 64, 7, 10, 64, 5, 3, 2),     # stride 3: nine classes, one launch each
    (3, 64, 6, 6, 64, 3, 1, 1),      # one tile over three images
)
FWD_STEM = ((2, 3, 2, 2, 64, 7, 2, 3), (2, 3, 6, 10, 64, 7, 2, 3), (2, 3, 32, 32, 64, 7, 2, 3),  # space-to-depth
            (2, 3, 33, 32, 64, 7, 2, 3), (2, 3, 32, 33, 64, 7, 2, 3))                              # im2col
# 2065 tiles, two per workgroup: the last workgroup holds one tile, with 4 live rows of 128 (N 4) or 8 of
# 256 (N 8)
FWD_PERSISTENT = ((4, 64, 257, 257, 128, 1, 1, 0), (4, 192, 257, 257, 128, 1, 1, 0), (8, 64, 257, 257, 64, 1, 1, 0))
# conv2d_fwd_stats: one image per statistics group; rows per group 256 (narrow and wide tile), 128 * 3
# (wide tile, at Cout 64 half empty), 45 (the separate statistics pass)
STATS_SHAPES = ((64, 16, 16, 64), (64, 16, 16, 128), (64, 8, 48, 64), (64, 8, 48, 128), (64, 5, 9, 64))  # (Cin, H, W, Cout)
STATS_GROUPS = (1, 2, 3)


def stats_shape(s, groups):
    cin, h, w, cout = s
    return (groups, cin, h, w, cout, 3, 1, 1)


DGRAD_SHAPES = FWD_BORDERS + tuple(s for s in FWD_CHANNEL_TAILS if s[4] % 64 == 0)
DGRAD_BN_FUSED = ((2, 64, 16, 16, 64, 3, 1, 1), (2, 64, 32, 32, 64, 3, 2, 1), (2, 128, 16, 16, 64, 1, 1, 0))
DGRAD_BN_UNFUSED = (2, 64, 5, 9, 64, 3, 1, 1)  # 45 rows per image: no whole 256-row tile
# weight gradients: (N, H, W) of the OUTPUT grid (the reduction, M = N H W rows) x (Cin, k) x Cout;
# stride 1, pad k // 2, so the input has the same extent
WGRAD_M = {1: (1, 1, 1), 63: (1, 7, 9), 64: (1, 4, 16), 65: (1, 5, 13), 512: (2, 8, 32), 1025: (1, 25, 41),
           25600: (1, 128, 200)}
WGRAD_COLS = ((64, 1), (64, 3), (128, 3))  # R S C = 64, 576, 1152
WGRAD_COUT = (8, 64, 72, 128, 136)


def wgrad_shape(m, cols, cout):
    n, h, w = WGRAD_M[m]
    cin, k = cols
    return (n, cin, h, w, cout, k, 1, k // 2)


WGRAD_SHAPES = tuple(wgrad_shape(m, c, k) for m in WGRAD_M for c in WGRAD_COLS for k in WGRAD_COUT)

BF16_FWD_SHAPES = FWD_ROW_TAILS + FWD_CHANNEL_TAILS + FWD_DEPTH + FWD_BORDERS + FWD_STEM + FWD_PERSISTENT + \
    tuple(stats_shape(s, g) for s in STATS_SHAPES for g in STATS_GROUPS)
BF16_DGRAD_SHAPES = DGRAD_SHAPES + DGRAD_BN_FUSED + (DGRAD_BN_UNFUSED,)
# A quarter-integer needs rounding to bf16 only from 257 grid units on; with fewer than 64 products
# per output that is out of reach for all but a sliver of them.  The 2 x 2 stem image has 12 (4 pixels
# of 3 channels, every other tap is padding): for it only the exactness precondition is checked.
SHORT_K_SHAPES = ((2, 3, 2, 2, 64, 7, 2, 3),)


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def out_size(shape):
    N, Cin, H, W, Cout, k, stride, pad = shape
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def rows(t):
    """[N, C, H, W] -> [N H W, C] (a view of a channels-last tensor)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def from_rows(r, N, H, W):
    return r.reshape(N, H, W, r.shape[-1]).permute(0, 3, 1, 2)


def fwd_tile(cout, stat_rows=None):
    """conv.hip's output tile (rows, channels): 256 x 64 up to 64 channels (with statistics only when
    the group is a multiple of 256 rows), 128 x 128 otherwise"""
    narrow = cout <= 64 and (stat_rows is None or stat_rows % 256 == 0)
    return (256, 64) if narrow else (128, 128)


def wgrad_tile(cout):
    return (64, 256) if cout <= 64 else (128, 128)


def describe_site(m, ch, N, H, W, tile=None, dgrad_stride=None):
    """Row m of an [N H W, C] output as (n, h, w, channel), its tile and in-tile row; for a data
    gradient the parity class (h % stride, w % stride), whose rows the tiles run over."""
    n, r = divmod(m, H * W)
    h, w = divmod(r, W)
    s = f"(n={n}, h={h}, w={w}, channel={ch})"
    cm = m
    if dgrad_stride is not None:
        st = dgrad_stride
        a, b = h % st, w % st
        I, J = (H - a + st - 1) // st, (W - b + st - 1) // st
        cm = (n * I + h // st) * J + w // st
        s += f", parity class ({a}, {b})"
    if tile is not None:
        tm, tn = tile
        s += f", tile row {cm // tm}, tile column {ch // tn}, in-tile row {cm % tm}, in-tile column {ch % tn}"
    return s


# ------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------
def _gen(shape, seed):
    h = seed * 1000003 + 17
    for v in shape:
        h = (h * 131 + int(v)) % (2 ** 61 - 1)
    return torch.Generator().manual_seed(h)


def _nhwc(g, N, C, H, W, lo, hi):
    """integers in [lo, hi] as a channels-last bf16 [N, C, H, W]"""
    return torch.randint(lo, hi + 1, (N, H, W, C), generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)


def _put(t, device):
    return t.to(device).contiguous(memory_format=CL)


def exact_image(shape, seed=0, device="cpu", x_max=X_MAX):
    N, Cin, H, W = shape[:4]
    return _put(_nhwc(_gen(shape, seed), N, Cin, H, W, 0, x_max), device)


def exact_weight(shape, seed=0, device="cpu", lean="cout"):
    """[Cout, Cin, k, k] bf16 with KRSC memory: integers in [-3, 3] times 2^-2 whose signs agree with a
    per-channel sign with a per-channel probability in [0.75, 1].  The channel is the one the sum does
    NOT run over: the output channel for the forward (``lean="cout"``), the input channel for a data
    gradient (``lean="cin"``), so that the sums do not cancel."""
    Cin, Cout, k = shape[1], shape[4], shape[5]
    g = _gen(shape, seed + 101)
    per = (Cout, 1, 1, 1) if lean == "cout" else (1, 1, 1, Cin)
    mag = torch.randint(0, W_MAX + 1, (Cout, k, k, Cin), generator=g)
    p = 0.75 + 0.25 * torch.rand(per, generator=g)
    agree = torch.rand(Cout, k, k, Cin, generator=g) < p
    sign = torch.randint(0, 2, per, generator=g) * 2 - 1
    w = (mag * torch.where(agree, 1, -1) * sign).double() * GRID
    return _put(w.to(torch.bfloat16).permute(0, 3, 1, 2), device)


def dgrad_weight(shape, seed=0, device="cpu"):
    return exact_weight(shape, seed, device, lean="cin")


def exact_grad(shape, seed=0, device="cpu", signed=False):
    """the upstream gradient [N, Cout, P, Q]: integers in [0, 16] (data gradients, whose bf16 result must
    need rounding) or in [-8, 8] (weight gradients, whose fp32 result needs none)"""
    P, Q = out_size(shape)
    lo, hi = (-DY_MAX, DY_MAX) if signed else (0, X_MAX)
    return _put(_nhwc(_gen(shape, seed + 202), shape[0], shape[4], P, Q, lo, hi), device)


def exact_prefill(shape_like, seed, device="cpu"):
    """fp32 integers in [-8, 8] (an accumulator's earlier content)"""
    g = torch.Generator().manual_seed(seed * 7919 + 5)
    return torch.randint(-PRE_MAX, PRE_MAX + 1, tuple(shape_like), generator=g).float().to(device)


def check_exactness_precondition(a, b, K, extras=0.0, what=""):
    """max|a| max|b| K (+ epilogue operands) < 2^24 in grid units, operands on their grids: every
    partial sum of the products is an integer number of grid units below 2^24, hence exact in fp32.
    ``b`` is the operand on the 2^-2 grid (or an integer one); returns the total."""
    a, b = a.double(), b.double() / GRID
    assert bool((a == a.round()).all()) and bool((b == b.round()).all()), f"{what}: operands off the dyadic grid"
    total = float(a.abs().max()) * float(b.abs().max()) * K + float(extras) / GRID
    assert total < 2.0 ** 24, f"{what}: exactness precondition violated: {total} grid units"
    return total


def fwd_precondition(x, w, what=""):
    return check_exactness_precondition(x, w, w.shape[1] * w.shape[2] * w.shape[3], what=what)


def dgrad_precondition(dy, w, residual_max=0.0, what=""):
    return check_exactness_precondition(dy, w, w.shape[0] * w.shape[2] * w.shape[3], extras=residual_max, what=what)


def wgrad_precondition(dy, x, what=""):
    """dy and x integers: M products of at most 8 * 16 plus the pre-filled value, below 2^24"""
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    a, b = dy.double(), x.double()
    assert bool((a == a.round()).all()) and bool((b == b.round()).all()), f"{what}: operands off the integer grid"
    total = float(a.abs().max()) * float(b.abs().max()) * M + PRE_MAX
    assert total < 2.0 ** 24, f"{what}: exactness precondition violated: {total}"
    return total


@dataclass
class BnOperands:
    """A BatchNorm+ReLU in front of the conv, chosen so that the kernel's pre-activation
    fmaf(x, gamma rstd, beta - mean gamma rstd) and xhat = fmaf(x, rstd, -mean rstd) are exact and the
    pre-activation is never 0: mean and beta are integers + 1/2, rstd is 1 or 4, gamma +-1/2 or +-2, so
    gamma rstd = +-2^j with j in {-1, 1, 3} (never +-1) and, for an integer x, (x - mean) gamma rstd + beta
    is an odd number of quarters (j = -1) or of halves (j = 1, 3)."""
    x: torch.Tensor      # [N, Cin, H, W] bf16 integers in [0, 16]: the BN input
    y: torch.Tensor      # [N, Cin, H, W] bf16 integers in [-2, 2]: a BN output to take the mask from
    mean: torch.Tensor   # [groups, Cin] fp32
    rstd: torch.Tensor
    gamma: torch.Tensor  # [Cin]
    beta: torch.Tensor

    def pre64(self, groups):
        """the pre-activation [N H W, C] in fp64 and the magnitude of its three addends"""
        C = self.x.shape[1]
        xr = rows(self.x).double().reshape(groups, -1, C)
        sc = self.gamma.double() * self.rstd.double()[:, None]
        mean, beta = self.mean.double()[:, None], self.beta.double()
        pre = (xr - mean) * sc + beta
        mag = (xr * sc).abs() + (mean * sc).abs() + beta.abs()
        return pre.reshape(-1, C), mag.reshape(-1, C)

    def live_from_x(self, groups):
        pre, _ = self.pre64(groups)
        assert bool((pre != 0).all()), "a pre-activation of exactly 0: the mask would depend on rounding"
        return pre > 0

    def undecided(self, groups):
        """real-valued operands: where the fp32 pre-activation (gamma rstd, beta - mean gamma rstd and one
        fmaf: four roundings of at most 2^-24 of the addends' magnitude) may fall on the other side of 0"""
        pre, mag = self.pre64(groups)
        return pre.abs() <= 4 * 2.0 ** -24 * mag

    def live_from_y(self):
        return rows(self.y).double() > 0

    def xhat_mag(self, groups):
        C = self.x.shape[1]
        xr = rows(self.x).double().reshape(groups, -1, C)
        rs = self.rstd.double()[:, None]
        return ((xr * rs).abs() + (self.mean.double()[:, None] * rs).abs()).reshape(-1, C)

    def xhat(self, groups):
        C = self.x.shape[1]
        xr = rows(self.x).double().reshape(groups, -1, C)
        return ((xr - self.mean.double()[:, None]) * self.rstd.double()[:, None]).reshape(-1, C)


def exact_bn(shape, groups, seed=0, device="cpu"):
    N, Cin, H, W = shape[:4]
    g = _gen(shape, seed + 303 + groups)
    x = _nhwc(g, N, Cin, H, W, 0, X_MAX)
    y = _nhwc(g, N, Cin, H, W, -2, 2)
    mean = torch.randint(0, X_MAX, (groups, Cin), generator=g).float() + 0.5
    rstd = torch.where(torch.rand(groups, Cin, generator=g) < 0.5, 1.0, 4.0)
    gamma = torch.where(torch.rand(Cin, generator=g) < 0.5, 0.5, 2.0) * (torch.randint(0, 2, (Cin,), generator=g) * 2 - 1)
    beta = torch.randint(-4, 4, (Cin,), generator=g).float() + 0.5
    return BnOperands(_put(x, device), _put(y, device), mean.to(device), rstd.to(device), gamma.float().to(device),
                      beta.to(device))


def real_bn(shape, groups, seed=0, device="cpu"):
    """randn-like BN operands for the bounded check (gamma of both signs, rstd in [0.5, 1.5])"""
    N, Cin, H, W = shape[:4]
    g = _gen(shape, seed + 505 + groups)
    x = torch.randn(N, H, W, Cin, generator=g).bfloat16().permute(0, 3, 1, 2)
    y = torch.randn(N, H, W, Cin, generator=g).bfloat16().permute(0, 3, 1, 2)
    mean = torch.randn(groups, Cin, generator=g) * 0.1
    rstd = torch.rand(groups, Cin, generator=g) + 0.5
    gamma = (torch.rand(Cin, generator=g) + 0.5) * (torch.randint(0, 2, (Cin,), generator=g) * 2 - 1)
    beta = torch.randn(Cin, generator=g) * 0.1
    return BnOperands(_put(x, device), _put(y, device), mean.to(device), rstd.to(device), gamma.float().to(device),
                      beta.to(device))


def real_problem(shape, seed=0, device="cpu"):
    """randn data for the bounded check: x, w / sqrt(K), dy"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    P, Q = out_size(shape)
    g = _gen(shape, seed + 404)
    x = torch.randn(N, H, W, Cin, generator=g).bfloat16().permute(0, 3, 1, 2)
    w = (torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5).bfloat16().permute(0, 3, 1, 2)
    dy = torch.randn(N, P, Q, Cout, generator=g).bfloat16().permute(0, 3, 1, 2)
    return _put(x, device), _put(w, device), _put(dy, device)


# ------------------------------------------------------------------------------------------------
# fp64 references (unfold / fold and one matmul; no convolution routine)
# ------------------------------------------------------------------------------------------------
def _pointwise(R, S, stride, pad):
    return R == 1 and S == 1 and stride == 1 and pad == 0


def ref_fwd64(x, w, stride, pad):
    """[N, Cout, P, Q] fp64"""
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    w2 = w.double().reshape(K, -1)  # columns in (c, r, s) order, as unfold's rows
    if _pointwise(R, S, stride, pad):
        return from_rows(torch.matmul(rows(x).double(), w2.t()), N, H, W)
    cols = F.unfold(x.double(), (R, S), padding=pad, stride=stride)  # [N, C R S, P Q]
    return torch.matmul(w2, cols).reshape(N, K, P, Q)


def ref_dgrad64(dy, w, stride, pad, H, W):
    """[N, Cin, H, W] fp64 (input pixels no window covers get 0)"""
    N, K, P, Q = dy.shape
    _, C, R, S = w.shape
    w2 = w.double().reshape(K, -1)
    if _pointwise(R, S, stride, pad):
        return from_rows(torch.matmul(rows(dy).double(), w2), N, H, W)
    cols = torch.matmul(w2.t(), dy.double().reshape(N, K, P * Q))  # [N, C R S, P Q]
    return F.fold(cols, (H, W), (R, S), padding=pad, stride=stride)


def ref_wgrad64(dy, x, R, S, stride, pad):
    """[Cout, Cin, R, S] fp64"""
    N, K, P, Q = dy.shape
    C = x.shape[1]
    cols = F.unfold(x.double(), (R, S), padding=pad, stride=stride)  # [N, C R S, P Q]
    d2 = dy.double().reshape(N, K, P * Q).permute(1, 0, 2).reshape(K, -1)
    c2 = cols.permute(1, 0, 2).reshape(C * R * S, -1)
    return torch.matmul(d2, c2.t()).reshape(K, C, R, S)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def _first_bad(got2, ref2):
    want = ref2.float().to(got2.dtype)
    bad = (gc._bits(got2) != gc._bits(want)).nonzero()
    return bad[0].tolist() if bad.numel() else None


def expect_exact_conv(got, ref64, what="", tile=None, dgrad_stride=None):
    """``got`` [N, C, H, W] bf16 against one rounding of ``ref64``, bit for bit (gemm_checks.expect_exact
    over the NHWC rows); a failure names the first differing (n, h, w, channel), its output tile and
    in-tile row and, for a data gradient (``dgrad_stride``), its parity class."""
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    N, C, H, W = got.shape
    g2, r2 = rows(got), rows(ref64)
    try:
        gc.expect_exact(g2, r2, what)
    except AssertionError as e:
        m, ch = _first_bad(g2, r2)
        raise AssertionError(f"{e}; first at {describe_site(m, ch, N, H, W, tile, dgrad_stride)}") from None


def expect_exact_wgrad(dw, ref64, what=""):
    """``dw`` [Cout, Cin, R, S] fp32 against ``ref64`` itself, bit for bit; a failure names the first
    differing (cout, r, s, cin) and its tile over the [Cout, R S Cin] matrix the kernel writes."""
    assert tuple(dw.shape) == tuple(ref64.shape), f"{what}: shape {tuple(dw.shape)} != {tuple(ref64.shape)}"
    K, C, R, S = dw.shape
    g2, r2 = dw.permute(0, 2, 3, 1).reshape(K, -1), ref64.permute(0, 2, 3, 1).reshape(K, -1)
    try:
        gc.expect_exact(g2, r2, what)
    except AssertionError as e:
        k, col = _first_bad(g2, r2)
        tm, tn = wgrad_tile(K)
        t, c = divmod(col, C)
        raise AssertionError(f"{e}; first at (cout={k}, r={t // S}, s={t % S}, cin={c}), tile row {k // tm}, tile column "
                             f"{col // tn}, in-tile row {k % tm}, in-tile column {col % tn}") from None


def record(name, worst, **fields):
    try:
        from conftest import record_margin

        record_margin(f"conv_elementwise[{name}]", worst_err_over_bound=worst, bound=1.0, **fields)
    except ImportError:
        pass


def expect_bounded_conv(got, ref64, abs64, K, what="", op="fwd", extras=0.0, rec=True):
    """gemm_checks.expect_bounded per element over the rows of a 4-D result (bf16 [N, C, H, W] outputs and
    data gradients, fp32 [Cout, Cin, R, S] weight gradients); records the worst err / bound."""
    out_bf16 = got.dtype == torch.bfloat16
    flat = (lambda t: rows(t)) if op != "wgrad" else (lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1))
    ex = flat(extras) if torch.is_tensor(extras) else extras
    worst = gc.expect_bounded(flat(got), flat(ref64), flat(abs64), K, out_bf16, ex, what, kernel="conv.hip " + op)
    if rec:  # (the CPU tier measures nothing worth keeping)
        record(what, worst, op=op, K=K, out_bf16=out_bf16)
    return worst


def expect_sum_of(got, before, terms64, what="", slack=0.0):
    """an fp32 accumulator (``before`` + the column sums of ``terms64`` [rows, C]) within
    rows 2^-24 sum |terms| per column (+ ``slack``): expect_colsum's bound for any column of addends"""
    n = terms64.shape[0]
    want = before.double() + terms64.sum(0)
    bound = n * 2.0 ** -24 * terms64.abs().sum(0) + slack
    bad = (got.double() - want).abs() > bound
    if bool(bad.any()):
        c = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} column sums off; first column {c}: got {float(got[c])}, want "
                             f"{float(want[c])} +- {float(bound[c])}")


def sum_is_exact(terms64, unit):
    """per column: every addend a multiple of ``unit`` and sum |terms| + 8 below 2^24 units, so that the
    fp32 sum, in any order and onto a pre-filled integer of at most 8, is the fp64 one"""
    q = terms64 / unit
    assert bool((q == q.round()).all()), "addends off the grid"
    return (q.abs().sum(0) + PRE_MAX / unit) < 2.0 ** 24


def expect_moments(sums, before, y, groups, what="", exact_too=True):
    """conv2d_fwd_stats' ``sums`` [groups][2][C] against the STORED output y [N, C, P, Q]: sum y within
    rows 2^-24 sum |y| (gemm_checks.expect_colsum) and sum y^2 within rows 2^-24 sum y^2.  Where a
    column's sum is exact in fp32 whatever the order (``sum_is_exact``; the stored values are multiples
    of 2^-2, their squares of 2^-4), it must equal the fp64 sum.  Returns how many (first, second)
    moments were exact."""
    C = y.shape[1]
    yr = rows(y).double().reshape(groups, -1, C)
    s, b = sums.reshape(groups, 2, C), before.reshape(groups, 2, C)
    n_exact = [0, 0]
    for g in range(groups):
        gc.expect_colsum(s[g, 0], b[g, 0], yr[g], f"{what} group {g} sum")
        expect_sum_of(s[g, 1], b[g, 1], yr[g] ** 2, f"{what} group {g} sum of squares")
        if exact_too:
            for mom, (terms, unit) in enumerate(((yr[g], GRID), (yr[g] ** 2, GRID * GRID))):
                ok = sum_is_exact(terms, unit)
                want = (b[g, mom].double() + terms.sum(0)).float()
                bad = ok & (s[g, mom] != want)
                assert not bool(bad.any()), (f"{what} group {g} moment {mom + 1}: an exact sum differs at channel "
                                             f"{int(bad.nonzero()[0])}")
                n_exact[mom] += int(ok.sum())
    return tuple(n_exact)


def expect_bn_bwd_sums(sums, before, g_stored, xhat64, groups, what="", xhat_mag64=None):
    """conv2d_dgrad_bn's ``sums`` [groups][2][C] against the STORED masked gradient g [N, C, H, W]:
    sum g and sum g xhat, each within rows 2^-24 sum |addend|.  On real-valued operands the kernel's
    fp32 xhat = fmaf(x, rstd, -mean rstd) is two roundings off the fp64 one: ``xhat_mag64`` =
    |x rstd| + |mean rstd| adds 2 * 2^-24 sum |g| xhat_mag to the second bound (exact operands: none)."""
    C = g_stored.shape[1]
    gr = rows(g_stored).double().reshape(groups, -1, C)
    xh = xhat64.reshape(groups, -1, C)
    s, b = sums.reshape(groups, 2, C), before.reshape(groups, 2, C)
    for g in range(groups):
        gc.expect_colsum(s[g, 0], b[g, 0], gr[g], f"{what} group {g} sum g")
        slack = 0.0 if xhat_mag64 is None else 2.0 ** -23 * (gr[g].abs() * xhat_mag64.reshape(groups, -1, C)[g]).sum(0)
        expect_sum_of(s[g, 1], b[g, 1], gr[g] * xh[g], f"{what} group {g} sum g xhat", slack)


def masked(g, live):
    """the stored bf16 gradient g [N, C, H, W] where ``live`` [N H W, C], +0 elsewhere, as fp64"""
    N, C, H, W = g.shape
    return from_rows(torch.where(live, rows(g).double(), 0.0), N, H, W)


def rel(a, b):
    """the whole-tensor metric of tests/test_conv.py (kept to show what it cannot see)"""
    return gc.rel(a, b)


def bf16_of(ref64):
    return ref64.float().bfloat16().contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------------
# planted corruptions (tests/test_conv_checks_cpu.py): each returns a damaged copy of a correct result
# ------------------------------------------------------------------------------------------------
def flip_one_ulp(out, n, ch, h, w):
    bad = out.clone()
    bad.view(torch.int16)[n, ch, h, w] += 1
    return bad


def zero_chunk(out, n, c8, h, w):
    """one 16-byte store (8 channels of one pixel) missing"""
    bad = out.clone()
    bad[n, c8 * 8:c8 * 8 + 8, h, w] = 0
    return bad


def replicated_pad_pixel(x, w, stride, pad, n, p, q):
    """the correct bf16 output except that the pixel (n, p, q) read its out-of-image taps from the
    nearest image pixel instead of zero"""
    bad = bf16_of(ref_fwd64(x, w, stride, pad))
    xp = F.pad(x.double(), (pad, pad, pad, pad), mode="replicate")
    bad[n, :, p, q] = ref_fwd64(xp, w, stride, 0)[n, :, p, q].float().bfloat16()
    return bad


def transposed_hw(x, w, stride, pad):
    """the bf16 output of a stride-1 same-size conv whose pixel decode swapped H and W: the image's
    memory read as [N, W, H, C], the result written as if it were [N, H, W, Cout]"""
    N, C, H, W = x.shape
    xb = from_rows(rows(x), N, W, H)
    yb = ref_fwd64(xb, w, stride, pad)
    assert yb.shape[2:] == (W, H), "same-size convs only"
    return bf16_of(from_rows(rows(yb), N, H, W))


def swapped_parity_classes(dx, stride, c0, c1):
    """a strided data gradient whose parity classes c0 and c1 landed on each other's pixels"""
    bad = dx.clone()
    (a0, b0), (a1, b1) = c0, c1
    bad[:, :, a0::stride, b0::stride] = dx[:, :, a1::stride, b1::stride]
    bad[:, :, a1::stride, b1::stride] = dx[:, :, a0::stride, b0::stride]
    return bad


def dropped_last_kstep(dy, x, R, S, stride, pad, before):
    """the weight gradient (accumulated onto ``before``) without the last 64-row step of the reduction
    (the rows from 64 floor((M - 1) / 64) on)"""
    N, K, P, Q = dy.shape
    d = rows(dy).clone()
    d[(d.shape[0] - 1) // 64 * 64:] = 0
    return (before.double() + ref_wgrad64(from_rows(d, N, P, Q), x, R, S, stride, pad)).float()


def moments_of_unrounded(ref64, before, groups):
    """``sums`` as a statistics epilogue would give them from the accumulators, before the bf16 store"""
    C = ref64.shape[1]
    yr = rows(ref64).reshape(groups, -1, C)
    return (before.reshape(groups, 2, C).double() + torch.stack([yr.sum(1), (yr * yr).sum(1)], 1)).float().reshape(-1)
