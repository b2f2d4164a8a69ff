"""Per-element checks of the training convolutions (csrc/kernels/conv.hip through conv2d_fwd,
conv2d_fwd_stats, conv2d_dgrad, conv2d_dgrad_bn, conv2d_wgrad and im2col_stem) at every tile, border
and epilogue.  Every case runs twice over: on exact data (tests/conv_checks.py: every partial sum exact
in fp32, so a bf16 output is bit-equal to one rounding of the fp64 reference and an fp32 weight
gradient to the reference; two runs bit-equal) and on randn data against the standard error bound
(full bf16 operands, the epilogues' real roundings).  References are fp64 unfold / fold + matmul on the
GPU from the bf16 operands.  One test per shape: all but the three persistent-forward cases are
sub-millisecond launches."""
import pytest
import torch

import conv_checks as cc
import gemm_checks as gc

pytestmark = pytest.mark.gpu


def _ids(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module")
def O():
    import dedloc_amd.ops  # noqa: F401

    return torch.ops.dedloc


def check_fwd(O, cuda, shape, seed=0):
    """conv2d_fwd on one shape: exact, repeatable, bounded; returns (x, w, y, ref64) of the exact problem"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    what = f"conv2d_fwd {shape}"
    x, w = cc.exact_image(shape, seed, cuda), cc.exact_weight(shape, seed, cuda)
    cc.fwd_precondition(x, w, what)
    ref = cc.ref_fwd64(x, w, stride, pad)
    y = O.conv2d_fwd(x, w, stride, pad)
    assert y.is_contiguous(memory_format=cc.CL)
    cc.expect_exact_conv(y, ref, what, tile=cc.fwd_tile(Cout))
    assert torch.equal(O.conv2d_fwd(x, w, stride, pad), y), f"{what}: two runs differ"
    rx, rw, _ = cc.real_problem(shape, seed, cuda)
    cc.expect_bounded_conv(O.conv2d_fwd(rx, rw, stride, pad), cc.ref_fwd64(rx, rw, stride, pad),
                           cc.ref_fwd64(rx.abs(), rw.abs(), stride, pad), Cin * k * k, f"fwd {shape}")
    return x, w, y, ref


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape", cc.FWD_ROW_TAILS, ids=_ids)
def test_fwd_row_tails(cuda, O, shape):
    """1x1 over a [1, 64, 1, m] image: one row short of, at and one past the 128- and 256-row tiles"""
    check_fwd(O, cuda, shape)


@pytest.mark.parametrize("shape", cc.FWD_CHANNEL_TAILS, ids=_ids)
def test_fwd_channel_tails(cuda, O, shape):
    """Cout 8 (one chunk), 64, 72, 128, 136, 192, 200: the narrow tile, the wide one and its tails"""
    check_fwd(O, cuda, shape)


@pytest.mark.parametrize("shape", cc.FWD_DEPTH, ids=_ids)
def test_fwd_pipeline_depth(cuda, O, shape):
    """nk = 1..5 k-steps: both parities of the two register stage sets, the clamped loads past the end"""
    check_fwd(O, cuda, shape)


@pytest.mark.parametrize("shape", cc.FWD_BORDERS, ids=_ids)
def test_fwd_borders_and_taps(cuda, O, shape):
    """non-square images smaller than, equal to and larger than the filter; pad 0, 1, 2, 3; stride 1, 2, 3"""
    check_fwd(O, cuda, shape)


@pytest.mark.parametrize("shape", cc.FWD_STEM, ids=_ids)
def test_fwd_stem(cuda, O, shape):
    """the 3-channel stem: space-to-depth at even sizes, the im2col matrix at odd H or W; with the
    column matrix handed in, the same bits"""
    x, w, y, _ = check_fwd(O, cuda, shape)
    cols = O.im2col_stem(x, 7, 7, 2, 3)
    assert torch.equal(O.conv2d_fwd(x, w, 2, 3, cols), y), f"stem {shape}: cols= changes the result"


@pytest.mark.parametrize("shape", cc.FWD_PERSISTENT, ids=_ids)
def test_fwd_persistent(cuda, O, shape):
    """2065 tiles, two per workgroup: the load cursor across the tile seam, the epilogue on alternating
    LDS buffers (Cin 64: every k-step ends a tile; Cin 192: odd nk, a seam inside the unrolled pair) and
    the last workgroup's single tile, of which 4 rows (N 4, 128-row tiles) or 8 rows (N 8, 256-row
    tiles) are live"""
    check_fwd(O, cuda, shape)


def test_fwd_refuses_partial_chunks(cuda, O):
    """conv.hip stores 8 channels (16 bytes) at a time: Cout 4 and 12 are refused before anything is
    launched, by the forward and (as input channels) by the data gradient"""
    for cout in (12, 4):
        shape = (1, 64, 5, 9, cout, 3, 1, 1)
        x, w = cc.exact_image(shape, 0, cuda), cc.exact_weight(shape, 0, cuda)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            O.conv2d_fwd(x, w, 1, 1)
        p1 = (1, 64, 1, 9, cout, 1, 1, 0)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            O.conv2d_fwd(cc.exact_image(p1, 0, cuda), cc.exact_weight(p1, 0, cuda), 1, 0)
        stem = (1, 3, 6, 10, cout, 7, 2, 3)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            O.conv2d_fwd(cc.exact_image(stem, 0, cuda), cc.exact_weight(stem, 0, cuda), 2, 3)
    back = (1, 12, 5, 9, 64, 3, 1, 1)  # a data gradient with 12 input channels
    with pytest.raises(RuntimeError, match="conv2d_dgrad"):
        O.conv2d_dgrad(cc.exact_grad(back, 0, cuda), cc.dgrad_weight(back, 0, cuda), 1, 1, 5, 9)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ forward + statistics
@pytest.mark.parametrize("groups", cc.STATS_GROUPS)
@pytest.mark.parametrize("s", cc.STATS_SHAPES, ids=_ids)
def test_fwd_stats(cuda, O, s, groups):
    """the statistics epilogue on the narrow tile (groups of 256 rows at Cout 64), on the wide tile (256
    rows at Cout 128; 128 * 3 rows at Cout 128 and, half empty, at Cout 64) and the separate statistics
    pass (45 rows): the output is conv2d_fwd's, the moments are those of the stored values and are
    added onto the buffer's content.  A first moment of the exact problem is an exact sum and must equal
    the fp64 one (hence repeat); second moments are exact sums only on the x in [0, 1] problem, and
    elsewhere, as on real data, are held to their bound."""
    shape = cc.stats_shape(s, groups)
    Cout, P, Q = shape[4], *cc.out_size(shape)
    what = f"conv2d_fwd_stats {shape}"
    tile = cc.fwd_tile(Cout, P * Q)
    x, w, y0, ref = check_fwd(O, cuda, shape)
    before = cc.exact_prefill((2 * groups * Cout,), groups, cuda)
    for run in range(2):
        sums = before.clone()
        y = O.conv2d_fwd_stats(x, w, 1, 1, sums, groups)
        assert torch.equal(y, y0), f"{what}: the output differs from conv2d_fwd's"
        cc.expect_exact_conv(y, ref, what, tile=tile)
        n1, _ = cc.expect_moments(sums, before, y, groups, f"{what} run {run}")
        assert n1 == groups * Cout  # every first moment is an exact sum: equal to the fp64 one in both runs
    # x in [0, 1]: exact second moments too
    xs = cc.exact_image(shape, 5, cuda, x_max=1)
    sums = before.clone()
    ys = O.conv2d_fwd_stats(xs, w, 1, 1, sums, groups)
    cc.expect_exact_conv(ys, cc.ref_fwd64(xs, w, 1, 1), what + " small", tile=tile)
    _, n2 = cc.expect_moments(sums, before, ys, groups, what + " small")
    assert n2 > 0 or P * Q != 256
    # real data: the same output as conv2d_fwd, inside the element bound; the moments of the stored values
    rx, rw, _ = cc.real_problem(shape, 0, cuda)
    sums = before.clone()
    ry = O.conv2d_fwd_stats(rx, rw, 1, 1, sums, groups)
    assert torch.equal(ry, O.conv2d_fwd(rx, rw, 1, 1)), f"{what}: the output differs from conv2d_fwd's on real data"
    cc.expect_bounded_conv(ry, cc.ref_fwd64(rx, rw, 1, 1), cc.ref_fwd64(rx.abs(), rw.abs(), 1, 1), shape[1] * 9,
                           f"fwd_stats {shape}", op="fwd_stats")
    cc.expect_moments(sums, before, ry, groups, what + " real", exact_too=False)


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("shape", cc.DGRAD_SHAPES, ids=_ids)
def test_dgrad(cuda, O, shape):
    """every geometry of the forward list with 64-multiple channel counts: parity classes of stride 2
    (merged launch; 1x1: three classes without a tap must come out as zeros) and stride 3 (one launch
    per class), with the per-class weights precomputed and with a residual"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    assert not (k == 1 and stride == 1 and pad == 0), "a pointwise data gradient may take a GEMM kernel"
    what = f"conv2d_dgrad {shape}"
    dy, w = cc.exact_grad(shape, 0, cuda), cc.dgrad_weight(shape, 0, cuda)
    cc.dgrad_precondition(dy, w, cc.X_MAX, what)
    ref = cc.ref_dgrad64(dy, w, stride, pad, H, W)
    dx = O.conv2d_dgrad(dy, w, stride, pad, H, W)
    assert dx.is_contiguous(memory_format=cc.CL)
    cc.expect_exact_conv(dx, ref, what, tile=cc.fwd_tile(Cin), dgrad_stride=stride)
    assert torch.equal(O.conv2d_dgrad(dy, w, stride, pad, H, W), dx), f"{what}: two runs differ"
    wds = O.conv2d_dgrad_weights(w, stride, pad)
    assert len(wds) == stride * stride
    assert torch.equal(O.conv2d_dgrad(dy, w, stride, pad, H, W, None, wds), dx), f"{what}: wds= changes the result"
    # off the GEMM route the residual is added to the stored gradient: a second rounding
    res = cc.exact_image(shape, 9, cuda)
    want = cc.bf16_of(ref).double() + res.double()
    cc.expect_exact_conv(O.conv2d_dgrad(dy, w, stride, pad, H, W, res, wds), want, what + " + residual",
                         tile=cc.fwd_tile(Cin), dgrad_stride=stride)
    _, rw, rdy = cc.real_problem(shape, 0, cuda)
    cc.expect_bounded_conv(O.conv2d_dgrad(rdy, rw, stride, pad, H, W), cc.ref_dgrad64(rdy, rw, stride, pad, H, W),
                           cc.ref_dgrad64(rdy.abs(), rw.abs(), stride, pad, H, W), Cout * k * k, f"dgrad {shape}",
                           op="dgrad")


def _dgrad_bn(O, shape, dy, w, bn, mask, sums, groups):
    N, Cin, H, W, Cout, k, stride, pad = shape
    return O.conv2d_dgrad_bn(dy, w, stride, pad, H, W, None, bn.x, bn.y if mask == "y" else None, bn.mean, bn.rstd,
                             bn.gamma, bn.beta, sums, groups, None)


@pytest.mark.parametrize("mask", ("x", "y"))
@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("shape", cc.DGRAD_BN_FUSED, ids=_ids)
def test_dgrad_bn(cuda, O, shape, groups, mask):
    """the BN-backward epilogue of conv.hip, mask from the BN input (y=None) and from a given y: the
    masked gradient against the fp64 data gradient (not the kernel's own), the two sums against the
    stored gradient.  No GEMM kernel may take a call: the 1x1 case has 128 input channels, which gemm8's
    BN-backward epilogue (columns in multiples of 256) declines, so it too runs on conv.hip."""
    N, Cin, H, W, Cout, k, stride, pad = shape
    what = f"conv2d_dgrad_bn {shape} groups={groups} mask={mask}"
    tile = (256, 64) if Cin <= 64 else (128, 128)
    dy, w, bn = cc.exact_grad(shape, 0, cuda), cc.dgrad_weight(shape, 0, cuda), cc.exact_bn(shape, groups, 0, cuda)
    cc.dgrad_precondition(dy, w, what=what)
    live = bn.live_from_y() if mask == "y" else bn.live_from_x(groups)
    want = cc.masked(cc.bf16_of(cc.ref_dgrad64(dy, w, stride, pad, H, W)), live)
    before = cc.exact_prefill((2 * groups * Cin,), 3, cuda)
    runs = []
    for _ in range(2):
        sums = before.clone()
        with gc.took(what):  # no GEMM launch
            g, fused = _dgrad_bn(O, shape, dy, w, bn, mask, sums, groups)
        assert fused is True, what
        runs.append((g, sums))
    cc.expect_exact_conv(g, want, what, tile=tile, dgrad_stride=stride)
    assert torch.equal(runs[0][0], runs[1][0]), f"{what}: two runs differ"
    for _, sums in runs:
        cc.expect_bn_bwd_sums(sums, before, g, bn.xhat(groups), groups, what)
    gr = cc.rows(g).double().reshape(groups, -1, Cin)
    exact = torch.stack([cc.sum_is_exact(gr[i], cc.GRID) for i in range(groups)])
    s0, s1 = (s.reshape(groups, 2, Cin)[:, 0] for _, s in runs)
    assert bool(exact.any()) and torch.equal(s0[exact], s1[exact]), f"{what}: exact sums differ between two runs"
    want0 = (before.reshape(groups, 2, Cin)[:, 0].double() + gr.sum(1)).float()
    assert torch.equal(s0[exact], want0[exact]), f"{what}: an exact sum of g differs from the fp64 one"

    # real data.  Where the fp32 pre-activation may round to the other side of 0 (mask from x only), the
    # mask the kernel chose is taken: a zero there is accepted, as is the gradient.
    _, rw, rdy = cc.real_problem(shape, 0, cuda)
    rbn = cc.real_bn(shape, groups, 0, cuda)
    sums = before.clone()
    with gc.took(what + " real"):
        rg, fused = _dgrad_bn(O, shape, rdy, rw, rbn, mask, sums, groups)
    assert fused is True, what
    if mask == "y":
        rlive = rbn.live_from_y()
    else:
        pre, _ = rbn.pre64(groups)
        undecided = rbn.undecided(groups)
        assert float(undecided.double().mean()) < 1e-3
        rlive = torch.where(undecided, cc.rows(rg) != 0, pre > 0)
    assert 0.2 < float(rlive.double().mean()) < 0.8
    ref = cc.ref_dgrad64(rdy, rw, stride, pad, H, W)
    absr = cc.ref_dgrad64(rdy.abs(), rw.abs(), stride, pad, H, W)
    zero = torch.zeros((), dtype=torch.float64, device=ref.device)
    mref = cc.from_rows(torch.where(rlive, cc.rows(ref), zero), N, H, W)
    mabs = cc.from_rows(torch.where(rlive, cc.rows(absr), zero), N, H, W)
    cc.expect_bounded_conv(rg, mref, mabs, Cout * k * k, f"dgrad_bn {shape} groups={groups} mask={mask}", op="dgrad_bn")
    cc.expect_bn_bwd_sums(sums, before, rg, rbn.xhat(groups), groups, what + " real", xhat_mag64=rbn.xhat_mag(groups))


@pytest.mark.parametrize("groups", (1, 2))
def test_dgrad_bn_unfused(cuda, O, groups):
    """45 rows per image: no whole 256-row tile per group, so the plain unmasked gradient comes back,
    fused is False and the sums are untouched; on exact and on real data"""
    shape = cc.DGRAD_BN_UNFUSED
    N, Cin, H, W, Cout, k, stride, pad = shape
    dy, w, bn = cc.exact_grad(shape, 0, cuda), cc.dgrad_weight(shape, 0, cuda), cc.exact_bn(shape, groups, 0, cuda)
    before = cc.exact_prefill((2 * groups * Cin,), 4, cuda)
    sums = before.clone()
    g, fused = _dgrad_bn(O, shape, dy, w, bn, "x", sums, groups)
    assert fused is False
    cc.expect_exact_conv(g, cc.ref_dgrad64(dy, w, stride, pad, H, W), f"conv2d_dgrad_bn unfused {shape}",
                         tile=cc.fwd_tile(Cin), dgrad_stride=stride)
    assert torch.equal(sums, before)
    _, rw, rdy = cc.real_problem(shape, 0, cuda)
    rg, fused = _dgrad_bn(O, shape, rdy, rw, cc.real_bn(shape, groups, 0, cuda), "x", sums, groups)
    assert fused is False and torch.equal(sums, before)
    cc.expect_bounded_conv(rg, cc.ref_dgrad64(rdy, rw, stride, pad, H, W),
                           cc.ref_dgrad64(rdy.abs(), rw.abs(), stride, pad, H, W), Cout * k * k,
                           f"dgrad_bn unfused {shape} groups={groups}", op="dgrad_bn")


# ------------------------------------------------------------------------------------------------ weight gradient
def check_wgrad(O, cuda, shape, nchw=False, tag=""):
    N, Cin, H, W, Cout, k, stride, pad = shape
    what = f"conv2d_wgrad {shape} nchw={nchw}"
    dy, x = cc.exact_grad(shape, 0, cuda, signed=True), cc.exact_image(shape, 0, cuda)
    cc.wgrad_precondition(dy, x, what)
    before = cc.exact_prefill((Cout, k, k, Cin), Cout + k, cuda).permute(0, 3, 1, 2)  # KRSC memory
    if nchw:
        before = before.contiguous()
    want = before.double() + cc.ref_wgrad64(dy, x, k, k, stride, pad)
    runs = []
    for _ in range(2):
        dw = before.clone()
        assert dw.stride() == before.stride()
        O.conv2d_wgrad(dy, x, dw, stride, pad)
        runs.append(dw)
    cc.expect_exact_wgrad(runs[0], want, what)
    assert torch.equal(runs[0], runs[1]), f"{what}: two runs differ"
    rx, _, rdy = cc.real_problem(shape, 0, cuda)
    dw = before.clone()
    O.conv2d_wgrad(rdy, rx, dw, stride, pad)
    cc.expect_bounded_conv(dw, before.double() + cc.ref_wgrad64(rdy, rx, k, k, stride, pad),
                           cc.ref_wgrad64(rdy.abs(), rx.abs(), k, k, stride, pad), N * H * W, f"wgrad {shape}{tag}",
                           op="wgrad", extras=before.double().abs())
    return runs[0]


@pytest.mark.parametrize("cout", cc.WGRAD_COUT)
@pytest.mark.parametrize("cols", cc.WGRAD_COLS, ids=lambda c: f"c{c[0]}k{c[1]}")
@pytest.mark.parametrize("m", tuple(cc.WGRAD_M))
def test_wgrad(cuda, O, m, cols, cout):
    """narrow (Cout 8, 64) and wide (72, 128, 136) kernels x 64, 576, 1152 gathered columns at a reduction
    of m rows: inside one k-step (1, 63, 64, 65), one split of 8 steps (512: the += path), two splits
    whose last step holds one row (1025: atomics), about 50 splits on the one-tile grids (25600), all
    onto a pre-filled dw"""
    check_wgrad(O, cuda, cc.wgrad_shape(m, cols, cout))


@pytest.mark.parametrize("cout", (64, 136))
@pytest.mark.parametrize("m", (65, 1025))
def test_wgrad_nchw_destination(cuda, O, m, cout):
    """an NCHW-contiguous dw goes through a KRSC temporary"""
    check_wgrad(O, cuda, cc.wgrad_shape(m, cc.WGRAD_COLS[1], cout), nchw=True, tag=" nchw")


def test_wgrad_single_split_mode_same_bits(cuda, O, monkeypatch):
    """DEDLOC_DETERMINISTIC_BN=1 runs the reduction as one split: on exact data the same bits"""
    shape = cc.wgrad_shape(1025, cc.WGRAD_COLS[1], 72)
    split = check_wgrad(O, cuda, shape)
    monkeypatch.setenv("DEDLOC_DETERMINISTIC_BN", "1")
    assert torch.equal(check_wgrad(O, cuda, shape, tag=" single split"), split)
