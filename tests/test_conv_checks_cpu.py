"""The convolution checker (tests/conv_checks.py) against the CPU implementations of the same operators:
the exact generators and checks accept a correct result, catch each planted localized corruption (and
where the older whole-tensor ``_rel < 1e-2`` of tests/test_conv.py misses it, that is asserted too), the
failure report names pixel, tile and parity class, and the generator's two promises (exactness in
fp32, at least 10 % of the bf16 outputs needing rounding) hold on every shape the GPU tier
(tests/test_conv_exact_gpu.py) runs — so that tier cannot be vacuous."""
import pytest
import torch
import torch.nn.functional as F

import conv_checks as cc
import dedloc_amd.ops  # noqa: F401
import gemm_checks as gc

OPS = torch.ops.dedloc
BIG_ROWS = 1 << 16  # above this many output rows the rounding share is taken on the first image only


def _ids(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------------------ generator promises
def test_forward_shapes_are_exact_and_need_rounding():
    worst = 0.0
    for shape in cc.BF16_FWD_SHAPES:
        x, w = cc.exact_image(shape), cc.exact_weight(shape)
        worst = max(worst, cc.fwd_precondition(x, w, f"fwd {shape}"))
        if shape in cc.SHORT_K_SHAPES:
            continue
        P, Q = cc.out_size(shape)
        xs = x[:1] if shape[0] * P * Q > BIG_ROWS else x
        gc.check_rounding_floor(cc.ref_fwd64(xs, w, shape[6], shape[7]), f"fwd {shape}")
    assert worst <= 16 * 3 * 9 * 512  # the bound of the largest 3x3 conv of the trunk, far below 2^24


def test_data_gradient_shapes_are_exact_and_need_rounding():
    for shape in cc.BF16_DGRAD_SHAPES:
        dy, w = cc.exact_grad(shape), cc.dgrad_weight(shape)
        cc.dgrad_precondition(dy, w, residual_max=cc.X_MAX, what=f"dgrad {shape}")
        if shape in cc.SHORT_K_SHAPES:
            continue
        gc.check_rounding_floor(cc.ref_dgrad64(dy, w, shape[6], shape[7], shape[2], shape[3]), f"dgrad {shape}")


def test_weight_gradient_shapes_are_exact():
    for shape in cc.WGRAD_SHAPES:
        # operands only: the precondition reads their extrema and the reduction length
        cc.wgrad_precondition(cc.exact_grad(shape, signed=True), cc.exact_image(shape), f"wgrad {shape}")


def test_small_magnitude_statistics_problem_has_exact_second_moments():
    """x in [0, 1]: a share of the second moments of a 256-row group (and every first moment) is an exact
    fp32 sum in any order, so the GPU tier's equality of an exact moment with the fp64 sum is not
    vacuous for second moments"""
    shape = cc.stats_shape(cc.STATS_SHAPES[0], 2)
    x, w = cc.exact_image(shape, seed=5, x_max=1), cc.exact_weight(shape, seed=5)
    y = cc.bf16_of(cc.ref_fwd64(x, w, 1, 1))
    yr = cc.rows(y).double().reshape(2, 256, 64)
    for g in range(2):
        assert bool(cc.sum_is_exact(yr[g], cc.GRID).all())
        assert float(cc.sum_is_exact(yr[g] ** 2, cc.GRID ** 2).double().mean()) >= 0.1


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("shape", cc.FWD_BORDERS + cc.FWD_STEM[:2] + cc.FWD_DEPTH[:1], ids=_ids)
def test_references_match_double_convolutions(shape):
    """unfold / fold + matmul against torch's own double convolutions (exact data: equality)"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    x, w = cc.exact_image(shape), cc.exact_weight(shape)
    assert torch.equal(cc.ref_fwd64(x, w, stride, pad), F.conv2d(x.double(), w.double(), stride=stride, padding=pad))
    dy = cc.exact_grad(shape)
    dx = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), stride=stride, padding=pad)
    assert torch.equal(cc.ref_dgrad64(dy, w, stride, pad, H, W), dx)
    dys = cc.exact_grad(shape, signed=True)
    dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, dys.double(), stride=stride, padding=pad)
    assert torch.equal(cc.ref_wgrad64(dys, x, k, k, stride, pad), dw)


# ------------------------------------------------------------------------------------------------ the CPU operators pass
@pytest.mark.parametrize("shape", cc.FWD_CHANNEL_TAILS[:3] + cc.FWD_BORDERS + cc.FWD_STEM[:2] + cc.FWD_ROW_TAILS[3:4], ids=_ids)
def test_exact_forward_passes_on_cpu_ops(shape):
    stride, pad = shape[6], shape[7]
    x, w = cc.exact_image(shape), cc.exact_weight(shape)
    ref = cc.ref_fwd64(x, w, stride, pad)
    cc.expect_exact_conv(OPS.conv2d_fwd(x, w, stride, pad), ref, f"conv2d_fwd {shape}", tile=cc.fwd_tile(shape[4]))
    rx, rw, _ = cc.real_problem(shape)
    worst = cc.expect_bounded_conv(OPS.conv2d_fwd(rx, rw, stride, pad), cc.ref_fwd64(rx, rw, stride, pad),
                                   cc.ref_fwd64(rx.abs(), rw.abs(), stride, pad), shape[1] * shape[5] ** 2,
                                   f"cpu fwd {shape}", rec=False)
    assert worst <= 1.0


@pytest.mark.parametrize("groups", cc.STATS_GROUPS)
def test_exact_forward_statistics_pass_on_cpu_ops(groups):
    for s in cc.STATS_SHAPES[:1] + cc.STATS_SHAPES[-1:]:
        shape = cc.stats_shape(s, groups)
        x, w = cc.exact_image(shape), cc.exact_weight(shape)
        before = cc.exact_prefill((2 * groups * shape[4],), seed=groups)
        sums = before.clone()
        y = OPS.conv2d_fwd_stats(x, w, 1, 1, sums, groups)
        cc.expect_exact_conv(y, cc.ref_fwd64(x, w, 1, 1), f"conv2d_fwd_stats {shape}")
        n1, _ = cc.expect_moments(sums, before, y, groups, f"conv2d_fwd_stats {shape}")
        assert n1 == groups * shape[4]  # every first moment of these shapes is an exact sum


@pytest.mark.parametrize("shape", cc.FWD_BORDERS, ids=_ids)
def test_exact_data_gradient_passes_on_cpu_ops(shape):
    N, Cin, H, W, Cout, k, stride, pad = shape
    dy, w = cc.exact_grad(shape), cc.dgrad_weight(shape)
    ref = cc.ref_dgrad64(dy, w, stride, pad, H, W)
    cc.expect_exact_conv(OPS.conv2d_dgrad(dy, w, stride, pad, H, W), ref, f"conv2d_dgrad {shape}",
                         tile=cc.fwd_tile(Cin), dgrad_stride=stride)
    res = cc.exact_image(shape, seed=9)
    # the CPU operator adds the residual before its one rounding
    cc.expect_exact_conv(OPS.conv2d_dgrad(dy, w, stride, pad, H, W, res), ref + res.double(), f"conv2d_dgrad+res {shape}")


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("mask", ("x", "y"))
def test_exact_bn_backward_gradient_passes_on_cpu_ops(groups, mask):
    shape = cc.DGRAD_BN_FUSED[0]
    N, Cin, H, W, Cout, k, stride, pad = shape
    dy, w, bn = cc.exact_grad(shape), cc.dgrad_weight(shape), cc.exact_bn(shape, groups)
    before = cc.exact_prefill((2 * groups * Cin,), seed=3)
    sums = before.clone()
    g, fused = OPS.conv2d_dgrad_bn(dy, w, stride, pad, H, W, None, bn.x, bn.y if mask == "y" else None, bn.mean, bn.rstd,
                                   bn.gamma, bn.beta, sums, groups, None)
    assert fused is True
    live = bn.live_from_y() if mask == "y" else bn.live_from_x(groups)
    assert 0.2 < float(live.double().mean()) < 0.8
    ref = cc.masked(cc.bf16_of(cc.ref_dgrad64(dy, w, stride, pad, H, W)), live)
    cc.expect_exact_conv(g, ref, f"conv2d_dgrad_bn mask={mask}", dgrad_stride=stride)
    cc.expect_bn_bwd_sums(sums, before, g, bn.xhat(groups), groups, f"conv2d_dgrad_bn mask={mask}")


@pytest.mark.parametrize("m", (1, 63, 64, 65, 512, 1025))
def test_exact_weight_gradient_passes_on_cpu_ops(m):
    for cols in cc.WGRAD_COLS[:2]:
        shape = cc.wgrad_shape(m, cols, 72)
        N, Cin, H, W, Cout, k, stride, pad = shape
        dy, x = cc.exact_grad(shape, signed=True), cc.exact_image(shape)
        before = cc.exact_prefill((Cout, k, k, Cin), seed=m).permute(0, 3, 1, 2)
        dw = before.clone()
        OPS.conv2d_wgrad(dy, x, dw, stride, pad)
        cc.expect_exact_wgrad(dw, before.double() + cc.ref_wgrad64(dy, x, k, k, stride, pad), f"conv2d_wgrad {shape}")


# ------------------------------------------------------------------------------------------------ planted corruptions
WIDE = (4, 64, 28, 40, 64, 3, 1, 1)    # a non-square image, 4480 output pixels
SQUARE = (4, 64, 28, 28, 64, 3, 1, 1)


@pytest.fixture(scope="module")
def wide():
    x, w = cc.exact_image(WIDE), cc.exact_weight(WIDE)
    ref = cc.ref_fwd64(x, w, 1, 1)
    return x, w, ref, cc.bf16_of(ref)


@pytest.fixture(scope="module")
def wide_real():
    """the same shape on the randn data of the older tests, for what their metric sees"""
    x, w, _ = cc.real_problem(WIDE)
    return x, w, cc.bf16_of(cc.ref_fwd64(x, w, 1, 1))


def _caught(bad, ref, **kw):
    with pytest.raises(AssertionError, match="elements differ"):
        cc.expect_exact_conv(bad, ref, "planted", **kw)


def test_flipped_ulp_caught_and_missed_by_rel(wide):
    _, _, ref, good = wide
    bad = cc.flip_one_ulp(good, 3, 63, 27, 39)
    _caught(bad, ref)
    assert cc.rel(bad, good) < 1e-2


def test_zeroed_chunk_caught_and_missed_by_rel(wide, wide_real):
    _, _, ref, good = wide
    bad = cc.zero_chunk(good, 2, 5, 13, 21)
    assert not torch.equal(bad, good)
    _caught(bad, ref)
    assert cc.rel(bad, good) < 1e-2
    _, _, rgood = wide_real
    assert cc.rel(cc.zero_chunk(rgood, 2, 5, 13, 21), rgood) < 1e-2


def test_replicated_pad_pixel_caught_and_missed_by_rel(wide, wide_real):
    """an edge pixel that read its three out-of-image taps from the image's own border row"""
    x, w, ref, good = wide
    bad = cc.replicated_pad_pixel(x, w, 1, 1, 1, 0, 17)
    assert not torch.equal(bad, good) and torch.equal(bad[:, :, 1:], good[:, :, 1:])
    _caught(bad, ref)
    rx, rw, rgood = wide_real
    rbad = cc.replicated_pad_pixel(rx, rw, 1, 1, 1, 0, 17)
    assert not torch.equal(rbad, rgood)
    assert cc.rel(rbad, rgood) < 1e-2


def test_transposed_image_caught_and_invisible_on_a_square_one(wide):
    x, w, ref, good = wide
    bad = cc.transposed_hw(x, w, 1, 1)
    assert not torch.equal(bad, good)
    _caught(bad, ref)
    xs, ws = cc.exact_image(SQUARE), cc.exact_weight(SQUARE)
    # H == W: the swapped decode computes the right answer, which is all the square shapes of the
    # older tests can show
    assert torch.equal(cc.transposed_hw(xs, ws, 1, 1), cc.bf16_of(cc.ref_fwd64(xs, ws, 1, 1)))


def test_swapped_parity_classes_caught():
    shape = (2, 64, 8, 12, 64, 3, 2, 1)
    dy, w = cc.exact_grad(shape), cc.dgrad_weight(shape)
    ref = cc.ref_dgrad64(dy, w, 2, 1, 8, 12)
    good = cc.bf16_of(ref)
    cc.expect_exact_conv(good, ref, "correct", dgrad_stride=2)
    bad = cc.swapped_parity_classes(good, 2, (0, 1), (1, 0))
    with pytest.raises(AssertionError, match=r"parity class \((0, 1|1, 0)\)"):
        cc.expect_exact_conv(bad, ref, "planted", tile=cc.fwd_tile(64), dgrad_stride=2)


def test_dropped_last_kstep_caught():
    for m in (65, 1025):  # a last step of one row
        shape = cc.wgrad_shape(m, cc.WGRAD_COLS[1], 72)
        N, Cin, H, W, Cout, k, stride, pad = shape
        dy, x = cc.exact_grad(shape, signed=True), cc.exact_image(shape)
        before = cc.exact_prefill((Cout, k, k, Cin), seed=1).permute(0, 3, 1, 2)
        ref = before.double() + cc.ref_wgrad64(dy, x, k, k, stride, pad)
        cc.expect_exact_wgrad(ref.float(), ref, "correct")
        bad = cc.dropped_last_kstep(dy, x, k, k, stride, pad, before)
        with pytest.raises(AssertionError, match="elements differ"):
            cc.expect_exact_wgrad(bad, ref, "planted")


def test_statistics_of_unrounded_output_caught_and_missed_by_rel(wide):
    """sums taken from the accumulators instead of the stored bf16 values: inside the older tests'
    ``_rel(sums, ref) < 1e-4``, outside the per-column bound"""
    _, _, ref, good = wide
    groups = 2
    before = torch.zeros(2 * groups * 64)
    right = cc.moments_of_unrounded(good.double(), before, groups)
    cc.expect_moments(right, before, good, groups, "correct", exact_too=False)
    bad = cc.moments_of_unrounded(ref, before, groups)
    with pytest.raises(AssertionError, match="column sums off"):
        cc.expect_moments(bad, before, good, groups, "planted", exact_too=False)
    assert cc.rel(bad, right) < 1e-4


# ------------------------------------------------------------------------------------------------ failure reports
def test_failure_report_names_pixel_tile_and_class(wide):
    _, _, ref, good = wide
    with pytest.raises(AssertionError) as e:
        cc.expect_exact_conv(cc.zero_chunk(good, 2, 5, 13, 21), ref, "planted", tile=cc.fwd_tile(64))
    msg = str(e.value)
    m = (2 * 28 + 13) * 40 + 21
    assert "8 of 286720" in msg and "(n=2, h=13, w=21, channel=40)" in msg
    assert f"tile row {m // 256}, tile column 0, in-tile row {m % 256}, in-tile column 40" in msg

    shape = (2, 128, 7, 10, 64, 3, 2, 1)  # data gradient [2, 128, 7, 10]: class (1, 0) has 3 x 5 pixels per image
    dy, w = cc.exact_grad(shape), cc.dgrad_weight(shape)
    dref = cc.ref_dgrad64(dy, w, 2, 1, 7, 10)
    with pytest.raises(AssertionError) as e:
        cc.expect_exact_conv(cc.flip_one_ulp(cc.bf16_of(dref), 1, 100, 5, 6), dref, "planted", tile=cc.fwd_tile(128),
                             dgrad_stride=2)
    msg = str(e.value)
    assert "(n=1, h=5, w=6, channel=100), parity class (1, 0)" in msg
    assert f"tile row 0, tile column 0, in-tile row {(1 * 3 + 2) * 5 + 3}, in-tile column 100" in msg

    with pytest.raises(AssertionError) as e:
        bad = torch.zeros(136, 64, 3, 3)
        bad[130, 7, 2, 1] = 1.0
        cc.expect_exact_wgrad(bad, torch.zeros(136, 64, 3, 3, dtype=torch.float64), "planted")
    assert "(cout=130, r=2, s=1, cin=7), tile row 1, tile column 3, in-tile row 2, in-tile column 71" in str(e.value)
