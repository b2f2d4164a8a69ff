"""The GEMM checker (tests/gemm_checks.py) against the CPU implementations of the same operators:
the exact generators and ``expect_exact`` accept a correct output, catch each planted localized
corruption that the older whole-tensor ``rel < 1e-2`` cannot see, and the generator's two promises
(exactness in fp32, at least 10 % of the outputs needing rounding) hold on every shape the GPU tier
(tests/test_gemm_exact_gpu.py) runs — so that tier cannot be vacuous."""
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
import gemm_checks as gc

OPS = torch.ops.dedloc
SHAPES = ((300, 256, 128), (257, 512, 64), (37, 70, 96))


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_checks_pass_on_cpu_ops(shape):
    M, N, K = shape
    p = gc.exact_problem(M, N, K, bias=True, residual=True, c=False)
    ref = p.ref64()
    gc.expect_exact(OPS.gemm(p.a, p.b, p.bias, p.res, False, True, 0), ref, "gemm NT")
    gc.expect_exact(OPS.gemm(p.a, p.b.t().contiguous(), p.bias, p.res, False, False, 0), ref, "gemm NN")

    q = gc.exact_problem(M, N, K, seed=1, c=True)
    c = q.c.clone()
    OPS.gemm_acc_f32(q.a.t().contiguous(), q.b.t().contiguous(), c, True, False)
    gc.expect_exact(c, q.ref64(), "gemm_acc_f32 TN")

    g = gc.exact_problem(M, N, K, seed=2, a_max=3, bias=True, tilt=False)
    H, G = OPS.gemm_gelu(g.a, g.b, g.bias, False)
    gc.expect_exact(H, g.ref64(), "gemm_gelu H")
    gc.expect_ulp(G, gc.gelu_new64(H), "gemm_gelu G")

    d = gc.exact_problem(M, N, K, seed=3)
    D = gc.grid_values((M, N), 6, seed=4)
    pre = gc.grid_values((N,), 8, seed=5, grid=1.0, dtype=torch.float32)
    dbias = pre.clone()
    C = OPS.gemm_dmul(d.a, d.b.t().contiguous(), D, dbias, False)
    gc.expect_exact(C, d.ref64().float().bfloat16().double() * D.double(), "gemm_dmul C")
    gc.expect_colsum(dbias, pre, C, "gemm_dmul dbias")

    probs = [gc.exact_problem(M, N, K, seed=10 + i) for i in range(3)]
    a = torch.stack([x.a for x in probs])
    b = torch.stack([x.b.t() for x in probs])
    ref = torch.stack([x.ref64() for x in probs])
    gc.expect_exact(OPS.bmm(a, b, False), ref, "bmm bf16")
    gc.expect_exact(OPS.bmm(a, b, True), ref, "bmm fp32")


@pytest.fixture(scope="module")
def big():
    """A correct 1000 x 512 output (the size of the older ``test_mfma_gemm_nt_nn``) with a bias."""
    p = gc.exact_problem(1000, 512, 320, bias=True)
    return p, p.ref64().float().bfloat16()


def _caught(bad, p):
    with pytest.raises(AssertionError, match="elements differ"):
        gc.expect_exact(bad, p.ref64(), "planted", tile=gc.TILE)


def test_flipped_ulp_caught_and_missed_by_rel(big):
    p, good = big
    bad = gc.flip_one_ulp(good, 999, 511)
    _caught(bad, p)
    assert gc.rel(bad, good) < 1e-2


def test_zeroed_chunk_caught_and_missed_by_rel(big):
    p, good = big
    bad = gc.zero_chunk(good, 517, 33)
    assert not torch.equal(bad, good)
    _caught(bad, p)
    assert gc.rel(bad, good) < 1e-2


def test_shifted_bias_block_caught_and_missed_by_rel(big):
    p, good = big
    bad = gc.shift_bias_block(p, 9)
    assert not torch.equal(bad, good)
    _caught(bad, p)
    assert gc.rel(bad, good) < 1e-2


def test_duplicated_last_row_caught_and_missed_by_rel(big):
    """One whole wrong row of M independent ones moves ``rel`` by about sqrt(2 / M): 4.5 % at M = 1000,
    where the old metric does see it, and under 1 % from M = 20000 rows on — every GEMM of the real
    workload (262144 tokens).  So the miss is asserted on a 32768-row output, the catch on both."""
    p, good = big
    _caught(gc.duplicate_last_row(good), p)
    tall = gc.exact_problem(32768, 512, 64, tilt=False)
    out = tall.ref64().float().bfloat16()
    bad = gc.duplicate_last_row(out)
    assert not torch.equal(bad, out)
    _caught(bad, tall)
    assert gc.rel(bad, out) < 1e-2


def test_failure_report_names_the_tile(big):
    p, good = big
    with pytest.raises(AssertionError) as e:
        gc.expect_exact(gc.zero_chunk(good, 517, 33), p.ref64(), "planted", tile=gc.TILE)
    msg = str(e.value)
    assert "8 of 512000" in msg and "tile row 2, tile column 1, in-tile row 5, in-tile column 8" in msg


def test_bounded_check_catches_an_extra_rounding():
    """bf16(acc) rounded once too often (acc -> bf16 -> + R -> bf16) passes rel and fails the bound."""
    torch.manual_seed(0)
    a, b = torch.randn(300, 320).bfloat16(), torch.randn(512, 320).bfloat16()
    r = torch.randn(300, 512).bfloat16()
    p = gc.Exact(a, b, res=r)
    ref = p.ref64()
    good = ref.float().bfloat16()
    assert gc.expect_bounded(good, ref, p.abs_ab(), 320, True, p.extras(), "cpu good") <= 1.0
    twice = (torch.matmul(a.double(), b.double().t()).float().bfloat16().float() + r.float()).bfloat16()
    assert gc.rel(twice, good) < 1e-2
    with pytest.raises(AssertionError, match="err / bound"):
        gc.expect_bounded(twice, ref, p.abs_ab(), 320, True, p.extras(), "cpu rounded twice")


@pytest.mark.parametrize("variant", ["plain", "bias+residual"])
def test_rounding_floor_on_every_bf16_shape(variant):
    full = variant != "plain"
    worst = 1.0
    for (M, N, K) in gc.BF16_STORE_SHAPES:
        p = gc.exact_problem(M, N, K, bias=full, residual=full)  # asserts the exactness precondition
        worst = min(worst, gc.check_rounding_floor(p.ref64(), f"{variant} {(M, N, K)}"))
    assert worst >= gc.ROUNDING_FLOOR


def test_exactness_precondition_on_every_other_shape():
    for (M, N, K) in gc.SHORT_K_SHAPES + gc.SMALL_SHAPES:
        gc.exact_problem(M, N, K, bias=True, residual=True)
    for (T, M, N, _) in gc.WGRAD_TN:
        gc.exact_problem(M, N, T, a_max=3, c=True)
    gc.exact_problem(*gc.WGRAD_NT, c=True)
    gc.exact_problem(*gc.SHARED_SHAPE, a_max=3, c=True)
    for (_, M, N, K) in gc.BMM_SHAPES:
        gc.exact_problem(M, N, K)
    gc.exact_problem(*gc.SPLIT_DEFECT, a_max=1, b_max=1, grid=1.0, c=True)
    with pytest.raises(AssertionError, match="precondition"):
        gc.exact_problem(8, 8, 700000)
