"""Shared checks of the row kernels — layernorm.hip, elementwise.hip, embedding.hip, xent.hip and
optim.hip (tests/test_row_checks_cpu.py, tests/test_row_kernels_exact_gpu.py).

As in tests/gemm_checks.py every check is per element (a Frobenius-norm ratio cannot see one wrong
16-byte store, one repeated tail row or one dropped term of a column sum) and of two kinds:

* exact: integer-valued bf16 data in [-8, 8] over at most 4096 rows makes every partial column sum an
  integer below 2^24, exact in fp32 in any order and under any atomics order, so a column sum must be
  bit-equal to the fp64 sum; saved sums, casts and copies are bit-equal to one rounding.
* bounded: real-valued data against an fp64 reference from the same bf16 inputs, within a bound
  made of bf16's half ulp (2^-8 |ref|) and fp32 terms in u = 2^-24 (``expect_within``).

Operands come from a seeded host generator (the same values in both tiers) and are moved to the
device the caller names.  The ``run_*`` functions generate one case, call the operators and apply
every check; both tiers call them, the CPU tier on the CPU implementations of the operators."""
import math

import torch

from gemm_checks import (duplicate_last_row, expect_exact, expect_ulp, flip_one_ulp, gelu_new64,  # noqa: F401
                         gelu_new_grad64, rel, zero_chunk)

U = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8
EPS = 1e-12

# ------------------------------------------------------------------------------------------------
# the cases of the GPU tier; the CPU tier runs every one of them through the CPU operators
# ------------------------------------------------------------------------------------------------
LN_D = (64, 128, 256, 512, 768, 1024, 2048, 4096)
LN_FWD_ROWS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)        # a block is 4 waves x R rows, R = 1, 2, 4
LN_BWD_ROWS = (1, 7, 8, 9, 31, 33, 65, 97)              # nparts = clamp(rows / 32, 1, 512) = 1, 2, 3
LN_BWD_BIG = ((1000, 128), (1000, 768), (1000, 2048),   # nparts 31, rpb 33: a last block of 10 rows
              (1089, 128), (1089, 768), (1089, 2048))   # nparts 34, rpb 33: the last block owns no row
GELU_N = tuple(8 * k for k in (1, 255, 256, 257, 1023, 1024, 1025, 2049))  # 1024-vector block chunks
GELU_BWD_N = GELU_N + (4194304 + 8 * 257,)              # past the 2048-block grid cap
COLSUM_ROWS = (1, 7, 8, 9, 63, 64, 65, 129)             # 8 rows per wave, 64 per block
COLSUM_N = (8, 504, 512, 520, 1032)                     # 512 columns per block
COLSUM_SCALAR_N = (1, 2, 3, 255, 257)
COLSUM_SCALAR_ROWS = (1, 63, 65, 200)
TANH_N = (1, 255, 256, 257, 524365)                     # 2048 x 256 threads, then the grid stride
CAST_N = (1, 3, 4, 5, 1023, 1024, 1025, 2098183)        # 4-wide vectors, scalar tail, grid stride
EMBED_E = (64, 128, 256, 512)
EMBED_BS = ((1, 1), (1, 3), (3, 5), (2, 64), (5, 37))
EMBED_TT = ("none", "two", "four")
EMBED_HOT = (4, 128, 300)                               # (B, S, tokens sharing one id)
EMBED_PACKED_T = (64, 128, 192)
EMBED_VOCAB, EMBED_POSITIONS = 50, 160
XENT_SHAPES = ((9, 8), (9, 2), (5, 2047), (5, 2048), (5, 2056), (4, 31995), (4, 30000), (1, 16))
IGNORE = -100
OPT_SIZES = (1, 37, 255, 256, 257, 1000, 1001, 4096)
OPT_ZERO_P, OPT_ZERO_G = 1, 2                           # tensors with all-zero parameters / gradient
OPT_WD = (0.01, 0.01, 0.0, 0.01, 0.0, 0.01, 0.0, 0.01)  # the zero-gradient tensor has no decay: u = 0
OPT_CHUNK = 1000
OPT_GRAD_SCALES = (1.0, 1.0 / 128)
OPT_FACTOR = 8.0   # bound = 8 x the CPU operator's own worst error (another reduction tree, FMA contraction)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, amax=8, dtype=torch.bfloat16):
    return torch.randint(-amax, amax + 1, shape, generator=g).to(dtype)


def nonzero_ints(g, shape, amax=8):
    """fp32 integers in [-amax, amax] without 0: what an accumulating buffer starts from."""
    v = torch.randint(1, amax + 1, shape, generator=g)
    return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def as2d(t, width=8):
    """A view whose (row, column) names an element: [rows, D] for row data, else [n / width, width]
    (the 16-byte vector and the lane in it) or [1, n]."""
    if t.dim() >= 2:
        return t.reshape(-1, t.shape[-1])
    return t.reshape(-1, width) if t.numel() % width == 0 and t.numel() else t.reshape(1, -1)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
RECORD = True  # the planted-defect tests switch it off: their ratios are no margins


def _record(test, **fields):
    if not RECORD:
        return
    try:
        from conftest import record_margin

        record_margin(test, **fields)
    except ImportError:
        pass


def expect_within(got, ref64, bound, what, term="", record=True):
    """Per element |got - ref| <= bound (NaN fails).  Reports the first offending (row, column), got and
    wanted there, the count and the worst err / bound, which it records and returns."""
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    g2, r2 = as2d(got.double()), as2d(ref64)
    b2 = as2d(bound.expand_as(ref64) if isinstance(bound, torch.Tensor) else torch.full_like(ref64, bound))
    err = (g2 - r2).abs()
    ratio = torch.where(b2 > 0, err / b2.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    ratio = torch.where(torch.isnan(g2), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if record:
        _record(f"row_kernels[{what}]", term=term, worst_err_over_bound=worst,
                max_abs_err=float(err.nan_to_num(math.inf).max()) if err.numel() else 0.0, bound=1.0)
    bad = ~(ratio <= 1.0)
    if bool(bad.any()):
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst err / bound = "
                             f"{worst:.3f}; first (row {r}, column {c}): got {float(g2[r, c])!r}, want "
                             f"{float(r2[r, c])!r} +- {float(b2[r, c]):.3e}")
    return worst


def expect_bits(got, want, what):
    """Two tensors of one dtype bit for bit (a copy, an alias, a saved input)."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape)
    expect_exact(as2d(got), as2d(want).double(), what)


def expect_zero(got, what):
    """Every element +0 or -0."""
    expect_within(got, torch.zeros(got.shape, dtype=torch.float64, device=got.device), 0.0, what, "exact zero", record=False)


def expect_finite_ulp(got, ref64, what):
    """``expect_ulp`` (the correctly rounded bf16 value or its neighbour) after a NaN / inf test, which a
    comparison of errors alone would pass."""
    g2 = as2d(got)
    bad = ~torch.isfinite(g2.float())
    if bool(bad.any()):
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite elements; first (row {r}, column {c}): got "
                             f"{float(g2[r, c])}, want {float(as2d(ref64)[r, c])}")
    r2 = as2d(ref64)
    ratio = (g2.double() - r2).abs() / (2.0 ** -7 * r2.abs() + 2.0 ** -20)  # expect_ulp's bound
    _record(f"row_kernels[{what}]", term="one bf16 ulp: 2^-7 |ref| + 2^-20", worst_err_over_bound=float(ratio.max()),
            max_abs_err=float((g2.double() - r2).abs().max()), bound=1.0)
    expect_ulp(g2, r2, what)


def expect_colsum_exact(got, before, x, what):
    """An fp32 column sum of integer data onto integer ``before``: bit-equal to the fp64 sum."""
    want = before.double() + x.double().reshape(-1, x.shape[-1]).sum(0)
    assert float(want.abs().max()) < 2.0 ** 24 and bool((want == want.round()).all()), f"{what}: sums not exact in fp32"
    expect_exact(got.reshape(1, -1), want.reshape(1, -1), what)


def expect_colsum_terms(got, before, terms64, what, record=True):
    """An fp32 column sum of the given fp64 terms [rows, N] onto ``before``: within
    (rows + 1) u (sum |terms| + |before|) per column — one rounding of each term and ``rows`` additions
    in any order, the one onto ``before`` included (rows u sum |terms| alone leaves a one-row sum onto a
    non-zero buffer no room: its product and its addition each round once)."""
    rows = terms64.shape[0]
    want = before.double() + terms64.sum(0)
    bound = (rows + 1) * U * (terms64.abs().sum(0) + before.double().abs())
    return expect_within(got.reshape(1, -1), want.reshape(1, -1), bound.reshape(1, -1), what,
                         "(rows + 1) u (sum|term| + |before|)", record)


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
def ln_rows(g, rows, D, first_kind=0, scale_r=False):
    """[rows, D] fp32 rows of four kinds in turn: zero-mean; offset by +8 (mean >> spread); scaled by
    2^-20; near-constant (all 3 with one 4).  ``scale_r``: the residual's share of such a row (nothing
    for the near-constant one, so its sum keeps the pattern)."""
    t = torch.randn(rows, D, generator=g)
    for r in range(rows):
        kind = (r + first_kind) % 4
        if kind == 1 and not scale_r:
            t[r] += 8.0
        elif kind == 2:
            t[r] *= 2.0 ** -20
        elif kind == 3:
            t[r] = 0.0 if scale_r else 3.0
            if not scale_r:
                t[r, (7 * r + 5) % D] = 4.0
    return t


def ln_problem(rows, D, with_res, integer=False, device="cpu"):
    g = _gen(1, rows, D, with_res, integer)
    if integer:
        x = ints(g, (rows, D))
        r = ints(g, (rows, D)) if with_res else None
    else:
        x = ln_rows(g, rows, D, first_kind=rows + D // 64).bfloat16()
        r = ln_rows(g, rows, D, first_kind=rows + D // 64, scale_r=True).bfloat16() if with_res else None
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g)
    dev = torch.device(device)
    return x.to(dev), (r.to(dev) if with_res else None), gamma.to(dev), beta.to(dev)


def ln_stats64(s, eps=EPS):
    """fp64 mean, rstd, xhat and the row's mean |s| of the stored bf16 rows ``s`` (eps as fp32)."""
    sd = s.double()
    mean = sd.mean(-1)
    var = ((sd - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    return mean, rstd, (sd - mean[:, None]) * rstd[:, None], sd.abs().mean(-1)


def check_ln_fwd_outputs(y, mean, rstd, s, gamma, beta, what, integer=False, eps=EPS):
    """y, mean, rstd of a LayerNorm over the stored rows ``s`` (also the embedding kernels' outputs)."""
    rows, D = s.shape
    m64, r64, xh, A = ln_stats64(s, eps)
    k = (D + 16) * U
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32 and tuple(mean.shape) == (rows,) == tuple(rstd.shape)
    expect_within(mean.reshape(-1, 1), m64.reshape(-1, 1), (k * A).reshape(-1, 1), f"{what} mean", "(D+16) u A")
    if integer and D & (D - 1) == 0:
        expect_exact(mean.reshape(-1, 1), m64.reshape(-1, 1), f"{what} mean of integer rows")
    elif integer:  # D = 768: the sum is exact, 1 / D and the product round once each
        ulp = torch.exp2(torch.frexp(m64)[1].double() - 24.0)
        expect_within(mean.reshape(-1, 1), m64.reshape(-1, 1), ulp.reshape(-1, 1), f"{what} mean of integer rows", "1 ulp")
    expect_within(rstd.reshape(-1, 1), r64.reshape(-1, 1), (k * (1.0 + A * r64) * r64).reshape(-1, 1), f"{what} rstd",
                  "(D+16) u (1 + A rstd)")
    ga, be = gamma.double(), beta.double()
    ref = xh * ga + be
    bound = HALF_ULP_BF16 * ref.abs() + k * ga.abs() * (xh.abs() + (A * r64)[:, None]) + U * be.abs()
    expect_within(y, ref, bound, f"{what} y", "bf16 half ulp + (D+16) u |gamma| (|xhat| + A rstd) + u |beta|")


def run_ln_fwd(O, rows, D, with_res, device, integer=False):
    what = f"ln_fwd rows={rows} D={D} res={with_res}" + (" int" if integer else "")
    x, r, gamma, beta = ln_problem(rows, D, with_res, integer, device)
    x0, r0 = x.clone(), (r.clone() if with_res else None)
    y, s, mean, rstd = O.layernorm_fwd(x, r, gamma, beta, EPS)
    expect_bits(x, x0, f"{what} x untouched")
    if with_res:
        expect_bits(r, r0, f"{what} res untouched")
        expect_exact(s, (x.float() + r.float()).double(), f"{what} s")
    else:
        expect_bits(s, x, f"{what} s")
    check_ln_fwd_outputs(y, mean, rstd, s, gamma, beta, what, integer)
    return y, s, mean, rstd


def ln_bwd_problem(rows, D, integer=False, device="cpu"):
    """dy, the stored rows s with their statistics (fp64 rounded to fp32), gamma: the backward's inputs."""
    g = _gen(2, rows, D, integer)
    s = ln_rows(g, rows, D, first_kind=rows).bfloat16()
    dy = ints(g, (rows, D)) if integer else torch.randn(rows, D, generator=g).bfloat16()
    gamma = torch.rand(D, generator=g) + 0.5
    mean, rstd, _, _ = ln_stats64(s)
    dev = torch.device(device)
    return dy.to(dev), s.to(dev), gamma.to(dev), mean.float().to(dev), rstd.float().to(dev)


def ln_bwd_ref(dy, s, gamma, mean, rstd):
    """fp64 ds and its bound from the mean / rstd actually passed in."""
    D = s.shape[-1]
    r64 = rstd.double()[:, None]
    xh = (s.double() - mean.double()[:, None]) * r64
    gy = dy.double() * gamma.double()
    a = gy.mean(-1, keepdim=True)
    b = (gy * xh).mean(-1, keepdim=True)
    ref = r64 * (gy - a - xh * b)
    bound = HALF_ULP_BF16 * ref.abs() + (D + 16) * U * r64 * (gy.abs() + gy.abs().mean(-1, keepdim=True)
                                                            + xh.abs() * (gy * xh).abs().mean(-1, keepdim=True))
    return ref, bound


def check_ln_bwd(ds, dgamma, dbeta, dsum, before, dy, s, gamma, mean, rstd, what, integer=False):
    """``before`` = (dgamma, dbeta, dsum) as they were before the call (zeros where it overwrites)."""
    ref, bound = ln_bwd_ref(dy, s, gamma, mean, rstd)
    expect_within(ds, ref, bound, f"{what} ds", "bf16 half ulp + (D+16) u rstd (|gy| + mean|gy| + |xhat| mean|gy xhat|)")
    # xhat as the operator forms it — (s - mean) * rstd, one fp32 rounding each — so that the column sum
    # is held to the error of its own products and additions, like gemm_checks.expect_colsum's stored C
    xh32 = (s.float() - mean[:, None]) * rstd[:, None]
    expect_colsum_terms(dgamma, before[0], dy.double() * xh32.double(), f"{what} dgamma")
    if integer:
        expect_colsum_exact(dbeta, before[1], dy, f"{what} dbeta")
    else:
        expect_colsum_terms(dbeta, before[1], dy.double(), f"{what} dbeta")
    if dsum is not None:
        expect_colsum_terms(dsum, before[2], ds.double(), f"{what} dsum")  # of the operator's own stored ds


def run_ln_bwd(O, rows, D, accumulate, with_dsum, device, integer=False):
    what = f"ln_bwd rows={rows} D={D} acc={accumulate} dsum={with_dsum}" + (" int" if integer else "")
    dy, s, gamma, mean, rstd = ln_bwd_problem(rows, D, integer, device)
    g = _gen(3, rows, D)
    start = [nonzero_ints(g, (D,)).to(dy.device) for _ in range(3)]
    dgamma, dbeta = start[0].clone(), start[1].clone()
    dsum = start[2].clone() if with_dsum else None
    ds = O.layernorm_bwd(dy, s, gamma, mean, rstd, dgamma, dbeta, accumulate, dsum)
    zero = torch.zeros_like(start[0])
    before = (start[0] if accumulate else zero, start[1] if accumulate else zero, start[2])
    check_ln_bwd(ds, dgamma, dbeta, dsum, before, dy, s, gamma, mean, rstd, what, integer)
    return ds, dgamma, dbeta, dsum


# ------------------------------------------------------------------------------------------------
# elementwise.hip
# ------------------------------------------------------------------------------------------------
SPECIALS = (0.0, -0.0, 8.0, -8.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4)


def activations(g, shape, scale=3.0, device="cpu"):
    """randn * scale (bf16) with the saturation points at both ends of the array (a tail vector has them
    too): 0, -0, +-8, +-30, +-100, +-1e4."""
    x = (torch.randn(shape, generator=g) * scale).bfloat16()
    flat = x.reshape(-1)
    sp = torch.tensor(SPECIALS, dtype=torch.bfloat16)
    k = min(len(SPECIALS), flat.numel())
    flat[:k] = sp[:k]
    flat[flat.numel() - k:] = sp[:k].flip(0)
    return x.to(torch.device(device))


def run_gelu_fwd(O, n, device):
    h = activations(_gen(4, n), (n,), device=device)
    y = O.gelu_fwd(h)
    expect_finite_ulp(y, gelu_new64(h), f"gelu_fwd n={n}")
    sat = h.float().abs() >= 30
    assert torch.equal(y[sat].float(), h[sat].float().clamp_min(0.0)), f"gelu_fwd n={n}: saturation is not x or 0"
    return y


def run_gelu_bwd(O, n, device):
    g = _gen(5, n)
    h = activations(g, (n,), device=device)
    dy = torch.randn(n, generator=g).bfloat16().to(h.device)
    dh = O.gelu_bwd(dy, h)
    expect_finite_ulp(dh, dy.double() * gelu_new_grad64(h), f"gelu_bwd n={n}")
    sat = h.float().abs() >= 30
    want = torch.where(h[sat].float() > 0, dy[sat].float(), torch.zeros_like(dy[sat].float()))
    assert torch.equal(dh[sat].float(), want), f"gelu_bwd n={n}: the saturated derivative is not 1 or 0"
    return dh


def run_gelu_bwd_dbias(O, rows, N, device):
    what = f"gelu_bwd+dbias rows={rows} N={N}"
    g = _gen(6, rows, N)
    h = activations(g, (rows, N), device=device)
    dy = torch.randn(rows, N, generator=g).bfloat16().to(h.device)
    before = nonzero_ints(g, (N,)).to(h.device)
    dbias = before.clone()
    dh = O.gelu_bwd(dy, h, dbias)
    expect_finite_ulp(dh, dy.double() * gelu_new_grad64(h), f"{what} dh")
    expect_colsum_terms(dbias, before, dh.double(), f"{what} dbias")  # of the operator's own stored dh
    return dh, dbias, before


def run_bias_grad(O, rows, N, accumulate, device):
    what = f"bias_grad rows={rows} N={N} acc={accumulate}"
    g = _gen(7, rows, N)
    dy = ints(g, (rows, N)).to(torch.device(device))
    before = nonzero_ints(g, (N,)).to(dy.device)
    dbias = before.clone()
    O.bias_grad(dy, dbias, accumulate)
    expect_colsum_exact(dbias, before if accumulate else torch.zeros_like(before), dy, what)
    return dbias


def run_tanh(O, n, device):
    g = _gen(8, n)
    x = activations(g, (n,), scale=2.0, device=device)
    y = O.tanh_fwd(x)
    expect_finite_ulp(y, torch.tanh(x.double()), f"tanh_fwd n={n}")
    sat = x.float().abs() >= 30
    assert torch.equal(y[sat].float(), torch.sign(x[sat].float())), f"tanh_fwd n={n}: saturation is not +-1"
    dy = torch.randn(n, generator=g).bfloat16().to(x.device)
    dx = O.tanh_bwd(dy, y)
    expect_finite_ulp(dx, dy.double() * (1.0 - y.double() ** 2), f"tanh_bwd n={n}")  # from the operator's own y
    return y, dx


def cast_inputs(n, device="cpu"):
    """fp32 values of every exponent from random bits (finite, |x| >= 2^-126), with +-0, +-inf, the exact
    ties 1 + 2^-8 (to even: down) and 1 + 3 2^-8 (up), the largest floats (they round up to inf) and a NaN
    at both ends of the array."""
    g = _gen(9, n)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    x = bits.view(torch.float32).clone()
    x[~(torch.isfinite(x) & (x.abs() >= 2.0 ** -126))] = 1.0
    big = float(torch.finfo(torch.float32).max)
    sp = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), big, -big, math.inf, -math.inf, 0.0, -0.0,
                       math.nan, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23], dtype=torch.float32)
    k = min(sp.numel(), n)
    x[:k] = sp[:k]
    x[n - k:] = sp[:k].flip(0)
    return x.to(torch.device(device))


def check_cast(out, x, what):
    want = x.to(torch.bfloat16)
    nan = torch.isnan(x)
    assert bool((torch.isnan(out) == nan).all()), f"{what}: NaN must stay NaN, and only NaN"
    expect_bits(torch.where(nan, torch.zeros_like(out), out), torch.where(nan, torch.zeros_like(want), want), what)


def run_cast(O, n, device):
    x = cast_inputs(n, device)
    out = torch.full((n,), -7.0, dtype=torch.bfloat16, device=x.device)
    O.cast_bf16(x, out)
    check_cast(out, x, f"cast_bf16 n={n}")
    return out


# ------------------------------------------------------------------------------------------------
# embeddings
# ------------------------------------------------------------------------------------------------
def embed_problem(E, B, S, tt_mode, hot=0, packed=False, device="cpu"):
    """ids, tt (None | {0, 1} | {0..3}), pos (packed: arbitrary in-range int32), the fp32 tables (the type
    table has as many rows as there are types), gamma, beta.  ``hot``: that many tokens share id 7."""
    T = B * S
    g = _gen(10, E, B, S, EMBED_TT.index(tt_mode), hot, packed)
    ntypes = 4 if tt_mode == "four" else 2
    ids = torch.randint(0, EMBED_VOCAB, (T,), generator=g)
    if hot:
        ids[torch.randperm(T, generator=g)[:hot]] = 7
    tt = None if tt_mode == "none" else torch.randint(0, ntypes, (T,), generator=g)
    pos = torch.randint(0, EMBED_POSITIONS, (T,), generator=g).to(torch.int32) if packed else None
    w = torch.randn(EMBED_VOCAB, E, generator=g)
    p = torch.randn(EMBED_POSITIONS, E, generator=g)
    t = torch.randn(ntypes, E, generator=g)
    gamma = torch.rand(E, generator=g) + 0.5
    beta = torch.randn(E, generator=g)
    dev = torch.device(device)
    mv = lambda z: None if z is None else z.to(dev)  # noqa: E731
    return dict(ids=mv(ids), tt=mv(tt), pos=mv(pos), w=mv(w), p=mv(p), t=mv(t), gamma=mv(gamma), beta=mv(beta), S=S,
                ntypes=ntypes)


def embed_indices(q):
    T = q["ids"].numel()
    pos = q["pos"].long() if q["pos"] is not None else torch.arange(T, device=q["ids"].device) % q["S"]
    tt = q["tt"] if q["tt"] is not None else torch.zeros_like(q["ids"])
    return pos, tt


def run_embed_fwd(O, q, what):
    if q["pos"] is None:
        y, s, mean, rstd = O.embed_ln_fwd(q["ids"], q["tt"], q["w"], q["p"], q["t"], q["gamma"], q["beta"], q["S"], EPS)
    else:
        y, s, mean, rstd = O.embed_ln_pos_fwd(q["ids"], q["tt"], q["pos"], q["w"], q["p"], q["t"], q["gamma"], q["beta"], EPS)
    pos, tt = embed_indices(q)
    want = ((q["w"][q["ids"]] + q["p"][pos]) + q["t"][tt]).bfloat16()  # that order, in fp32
    expect_bits(s, want, f"{what} s")
    check_ln_fwd_outputs(y, mean, rstd, s, q["gamma"], q["beta"], what)
    return y, s, mean, rstd


def embed_grad_ref(ds, q, before):
    """fp64 (dwemb, dpemb, dtemb) = before + scatter of the rows of ds."""
    pos, tt = embed_indices(q)
    g = ds.double()
    return (before[0].double().index_add_(0, q["ids"], g), before[1].double().index_add_(0, pos, g),
            before[2].double().index_add_(0, tt, g))


def check_embed_bwd(grads, before, ds, q, what):
    for name, got, want in zip(("dwemb", "dpemb", "dtemb"), grads, embed_grad_ref(ds, q, before)):
        assert float(want.abs().max()) < 2.0 ** 24, f"{what}: sums not exact in fp32"
        expect_exact(got, want, f"{what} {name}")


def run_embed_bwd(O, q, what):
    T, E = q["ids"].numel(), q["w"].shape[1]
    g = _gen(11, T, E)
    dev = q["ids"].device
    ds = ints(g, (T, E)).to(dev)
    before = [nonzero_ints(g, tuple(q[k].shape)).to(dev) for k in ("w", "p", "t")]
    grads = [b.clone() for b in before]
    if q["pos"] is None:
        O.embed_bwd(ds, q["ids"], q["tt"], *grads, q["S"])
    else:
        O.embed_pos_bwd(ds, q["ids"], q["tt"], q["pos"], *grads)
    check_embed_bwd(grads, before, ds, q, what)
    return grads, before, ds


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
def xent_problem(M, V, pin=0, all_ignored=False, device="cpu"):
    """randn * 3 logits; row 0 labelled ``pin`` steps from column 0, row 1 column V - 1, row 2 ignored
    (M = 1: ``pin`` = 0 / 1 chooses column 0 / V - 1)."""
    g = _gen(12, M, V, pin)
    x = (torch.randn(M, V, generator=g) * 3).bfloat16()
    lab = torch.randint(0, V, (M,), generator=g)
    lab[0] = 0 if pin == 0 else V - 1
    if M > 1:
        lab[1] = V - 1 if pin == 0 else 0
    if M > 2:
        lab[2] = IGNORE
    if all_ignored:
        lab[:] = IGNORE
    dev = torch.device(device)
    return x.to(dev), lab.to(dev)


def xent_ref(x, lab):
    """fp64 (loss, gradient, its bound, the loss's bound)."""
    xd = x.double()
    valid = lab != IGNORE
    cnt = int(valid.sum())
    scale = 1.0 / cnt if cnt else 0.0
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(xd, -1)
    xl = xd.gather(1, safe[:, None]).squeeze(1)
    loss = ((lse - xl) * valid).sum() * scale
    p = torch.softmax(xd, -1)
    onehot = torch.zeros_like(p).scatter_(1, safe[:, None], 1.0)
    grad = (p - onehot) * valid[:, None] * scale
    gbound = HALF_ULP_BF16 * grad.abs() + 2.0 ** -16 * scale * (p + onehot) + 2.0 ** -120
    lbound = 2.0 ** -16 * float(((lse.abs() + xl.abs()) * valid).sum()) * scale
    return loss, grad, gbound, lbound, valid


def check_xent(loss, grad, x, lab, what):
    rl, rg, gb, lb, valid = xent_ref(x, lab)
    expect_within(grad, rg, gb, f"{what} grad", "bf16 half ulp + 2^-16 scale (p + onehot) + 2^-120")
    expect_zero(grad[~valid], f"{what} ignored rows")
    expect_within(loss.reshape(1, 1), rl.reshape(1, 1), torch.full((1, 1), lb, dtype=torch.float64, device=x.device),
                  f"{what} loss", "2^-16 mean(|lse| + |x_label|)")


def run_xent(O, M, V, pin, device, all_ignored=False):
    what = f"xent M={M} V={V} pin={pin}" + (" all ignored" if all_ignored else "")
    x, lab = xent_problem(M, V, pin, all_ignored, device)
    x0 = x.clone()
    loss, grad = O.xent_fwd_bwd(x, lab, False, IGNORE)
    expect_bits(x, x0, f"{what} logits untouched")
    check_xent(loss, grad, x, lab, what)
    xi = x.clone()
    loss_i, grad_i = O.xent_fwd_bwd(xi, lab, True, IGNORE)
    assert grad_i.data_ptr() == xi.data_ptr() and grad_i.shape == xi.shape, f"{what}: inplace gradient does not alias"
    expect_bits(grad_i, grad, f"{what} inplace grad")
    check_xent(loss_i, grad_i, x, lab, f"{what} inplace")  # the loss: rows added atomically, in any order
    if all_ignored:
        assert float(loss) == 0.0 and not bool(torch.isnan(grad.float()).any()), f"{what}: loss {float(loss)}"
        expect_zero(grad, f"{what} grad")
    return loss, grad


# ------------------------------------------------------------------------------------------------
# optimizers
# ------------------------------------------------------------------------------------------------
def chunks(sizes, wd, dev, chunk=OPT_CHUNK):
    """The flat layout's work list (tensor id, start, length) as the fused optimizers take it."""
    ct, cs, cl, offs, off = [], [], [], [], 0
    for i, n in enumerate(sizes):
        offs.append(off)
        for s in range(0, n, chunk):
            ct.append(i)
            cs.append(off + s)
            cl.append(min(chunk, n - s))
        off += n
    return (torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(cs, dtype=torch.int64, device=dev),
            torch.tensor(cl, dtype=torch.int32, device=dev), torch.tensor(wd, dtype=torch.float32, device=dev), offs)


def opt_state(seed):
    g = _gen(13, seed)
    n = sum(OPT_SIZES)
    offs = [sum(OPT_SIZES[:i]) for i in range(len(OPT_SIZES))]
    p = torch.randn(n, generator=g)
    p[offs[OPT_ZERO_P]:offs[OPT_ZERO_P] + OPT_SIZES[OPT_ZERO_P]] = 0.0
    grads = []
    for _ in range(3):
        gr = torch.randn(n, generator=g)
        gr[offs[OPT_ZERO_G]:offs[OPT_ZERO_G] + OPT_SIZES[OPT_ZERO_G]] = 0.0
        grads.append(gr)
    return p, grads, offs


LAMB = dict(lr=1.76e-3, b1=0.9, b2=0.999, eps=1e-6, clamp=10.0)
LARC = dict(lr=1e-3, momentum=0.9, trust=1e-3, eps=1e-8)


def lamb_replay64(p, g, m, v, offs, step, gs):
    """One step of _lamb_cpu's formula in fp64 from the fp32 state (p, m, v in place)."""
    h = LAMB
    bc = math.sqrt(1 - h["b2"] ** step) / (1 - h["b1"] ** step)
    for i, (o, n) in enumerate(zip(offs, OPT_SIZES)):
        sl = slice(o, o + n)
        gi = g[sl] * gs
        m[sl] = h["b1"] * m[sl] + (1 - h["b1"]) * gi
        v[sl] = h["b2"] * v[sl] + (1 - h["b2"]) * gi * gi
        u = m[sl] / (v[sl].sqrt() + h["eps"]) + float(torch.tensor(OPT_WD[i], dtype=torch.float32)) * p[sl]
        wn = min(max(float(p[sl].norm()), 0.0), h["clamp"])
        un = float(u.norm())
        trust = 1.0 if (wn == 0 or un == 0) else wn / un
        p[sl] = p[sl] - h["lr"] * bc * trust * u
    return h["lr"] * bc


def larc_replay64(p, g, buf, offs, first, clip, gs):
    h = LARC
    for i, (o, n) in enumerate(zip(offs, OPT_SIZES)):
        sl = slice(o, o + n)
        wd = float(torch.tensor(OPT_WD[i], dtype=torch.float32))
        pn, gn = float(p[sl].norm()), float((g[sl] * gs).norm())
        a = 1.0
        if pn != 0 and gn != 0:
            a = h["trust"] * pn / (gn + pn * wd + h["eps"])
            if clip:
                a = min(a / h["lr"], 1.0)
        d = (g[sl] * gs + wd * p[sl]) * a
        buf[sl] = d if first else h["momentum"] * buf[sl] + d
        p[sl] = p[sl] - h["lr"] * buf[sl]


def _opt_err(got, ref, scale):
    e = (got.double().cpu() - ref).abs()
    r = torch.where(scale > 0, e / scale.clamp_min(1e-300), torch.where(e > 0, math.inf, 0.0))
    r = torch.where(torch.isnan(got.double().cpu()), torch.full_like(r, math.inf), r)
    i = int(r.argmax())
    return float(r[i]), i


def run_optimizer(O, kind, gs, device, clip=False):
    """Three steps of LAMB or LARC-SGD on ``device`` and, beside it, on the CPU operator; after every
    step p, m, v / buf of both against one fp64 step from the state that the device run had before it
    (so errors do not compound across steps).  Normalised per element by |p_old| + |delta_ref| (p) or
    |ref| (m, v, buf); the bound is OPT_FACTOR x the CPU operator's worst.  Returns the figures."""
    what = f"{kind} grad_scale={gs:g}" + (" clip" if clip else "")
    p0, grads, offs = opt_state(0 if kind == "lamb" else 1)
    names = ("p", "m", "v") if kind == "lamb" else ("p", "buf")
    figures = []
    cpu = torch.device("cpu")
    dev = torch.device(device)
    state = {d: dict(p=p0.clone().to(d), m=torch.zeros_like(p0).to(d), v=torch.zeros_like(p0).to(d),
                     buf=torch.zeros_like(p0).to(d), norms=torch.zeros(2 * len(OPT_SIZES)).to(d),
                     ck=chunks(OPT_SIZES, OPT_WD, d)) for d in {cpu, dev}}
    for step in range(1, 4):
        g = grads[step - 1]
        # every run starts the step from the device run's state, so both are compared with one replay
        for k in ("p", "m", "v", "buf"):
            state[cpu][k] = state[dev][k].detach().to(cpu).clone()
        ref = {k: state[cpu][k].double().clone() for k in ("p", "m", "v", "buf")}
        p_old = ref["p"].clone()
        if kind == "lamb":
            lamb_replay64(ref["p"], g.double(), ref["m"], ref["v"], offs, step, gs)
        else:
            larc_replay64(ref["p"], g.double(), ref["buf"], offs, step == 1, clip, gs)
        scale = dict(p=p_old.abs() + (ref["p"] - p_old).abs(), m=ref["m"].abs(), v=ref["v"].abs(), buf=ref["buf"].abs())
        out = {}
        for d in ([cpu] if dev == cpu else [cpu, dev]):
            st = state[d]
            ct, cs, cl, twd, _ = st["ck"]
            if kind == "lamb":
                h = LAMB
                bc = math.sqrt(1 - h["b2"] ** step) / (1 - h["b1"] ** step)
                O.lamb_step(st["p"], g.to(d), st["m"], st["v"], ct, cs, cl, twd, st["norms"], h["b1"], h["b2"], h["eps"],
                            h["lr"] * bc, h["clamp"], gs)
            else:
                h = LARC
                O.larc_sgd_step(st["p"], g.to(d), st["buf"], ct, cs, cl, twd, st["norms"], h["lr"], h["momentum"],
                                h["trust"], h["eps"], clip, step == 1, gs)
            out[d] = {k: _opt_err(st[k], ref[k], scale[k]) for k in names}
        for k in names:
            cpu_worst = out[cpu][k][0]
            bound = OPT_FACTOR * cpu_worst
            got, at = out[dev][k]
            figures.append(dict(what=what, step=step, quantity=k, cpu_worst=cpu_worst, bound=bound, device_worst=got))
            _record(f"row_kernels[{what} step={step} {k}]", term="8 x the CPU operator's worst normalised error",
                    cpu_worst_err=cpu_worst, bound=bound, device_worst_err=got,
                    worst_err_over_bound=(got / bound if bound > 0 else (0.0 if got == 0 else math.inf)))
            if not got <= bound:
                t = max(i for i, o in enumerate(offs) if o <= at)
                raise AssertionError(f"{what} step {step}: {k} worst normalised error {got:.3e} above the bound {bound:.3e} "
                                     f"(8 x the CPU operator's {cpu_worst:.3e}); first at (tensor {t}, element "
                                     f"{at - offs[t]}): got {float(state[dev][k][at])!r}, want {float(ref[k][at])!r}")
    return figures


# ------------------------------------------------------------------------------------------------
# planted defects (tests/test_row_checks_cpu.py): each returns a damaged copy of a correct output
# ------------------------------------------------------------------------------------------------
def swap_in_neighbour(v, i):
    """One row's statistic replaced by its neighbour's."""
    bad = v.clone()
    bad[i] = v[i - 1]
    return bad


def drop_one_term(colsum, x, r, c):
    """The column sum with element (r, c) of ``x`` left out."""
    bad = colsum.clone()
    bad[c] -= x[r, c].float()
    return bad


def add_id_twice(dwemb, ds, ids, token):
    """The word-table gradient with one token's row of ds added twice."""
    bad = dwemb.clone()
    bad[ids[token]] += ds[token].float()
    return bad


def shift_label_column(grad, lab, row, scale):
    """The cross-entropy gradient with the label's -1 applied one column to the left."""
    bad = grad.float().clone()
    bad[row, lab[row]] += scale
    bad[row, lab[row] - 1] -= scale
    return bad.bfloat16()
