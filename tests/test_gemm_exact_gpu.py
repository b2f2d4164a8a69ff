"""Per-element checks of the three GEMM kernels (gemm8.hip, gemm.hip, gemm_small.hip) at every
tile, tail and epilogue: exact data (tests/gemm_checks.py: every partial sum exact in fp32, so a bf16
output is bit-equal to one rounding of the fp64 reference and an fp32 output to the reference),
one standard-error-bound test per kernel on randn data, and the kernel that took each call read from
the backend counters.  References are fp64 torch.matmul on the GPU from the bf16 operands.  Each test
loops over its shapes: all are sub-millisecond launches."""
import pytest
import torch

import gemm_checks as gc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
VARIANTS = ((False, False), (True, False), (True, True))  # (bias, residual)


@pytest.fixture(scope="module")
def O():
    import dedloc_amd.ops  # noqa: F401

    return torch.ops.dedloc


def store(O, p, form):
    """out = a b^T (+ bias) (+ res) through `gemm`: NT (b [N, K], K-inner), NN (b [K, N], K-outer) or
    TN (a [K, M] and b [K, N], both K-outer)."""
    a = p.a.t().contiguous() if form == "TN" else p.a
    b = p.b if form == "NT" else p.b.t().contiguous()
    return O.gemm(a, b, p.bias, p.res, form == "TN", form == "NT", 0)


def check_store(O, cuda, shapes, forms, backend, seed=0):
    for (M, N, K) in shapes:
        for form in forms:
            for bias, residual in VARIANTS:
                what = f"gemm {form} {(M, N, K)} bias={bias} residual={residual}"
                p = gc.exact_problem(M, N, K, seed=seed, bias=bias, residual=residual, device=cuda)
                with gc.took(what, **{backend: 1}):
                    out = store(O, p, form)
                gc.expect_exact(out, p.ref64(), what, tile=gc.TILE)


# ------------------------------------------------------------------------------------------------ gemm8 store
def test_gemm8_store_m_tails(cuda, O):
    """the epilogue's 8-row pass, 64-row quadrant and 128-row wave half, from both sides"""
    check_store(O, cuda, gc.GEMM8_TAIL_SHAPES, ("NT", "NN"), "gemm8")


def test_gemm8_store_pipeline_depth(cuda, O):
    """nk = 1..5 K-tiles: the prologue alone, each peeled tail, one steady iteration, both parities"""
    check_store(O, cuda, gc.GEMM8_DEPTH_SHAPES, ("NT", "NN"), "gemm8")


def test_gemm8_store_tile_order(cuda, O):
    """5 / 6 / 7 / 8 row blocks (last bands of 1 / 2 / 3 / 4) and 5 / 18 / 21 / 16 tiles"""
    check_store(O, cuda, gc.GEMM8_ORDER_SHAPES, ("NT", "NN"), "gemm8")


# ------------------------------------------------------------------------------------------------ fused epilogues
def _fused_backend(N, k_inner_b, own_epilogue=True):
    """gemm8 inside its contract (N % 256 == 0); else gemm.hip takes a K-inner B (fused bias + GELU, or
    the plain store of the unfused pair) and gemm_small a K-outer B whose N is no multiple of 256.
    An output of at most 192 columns reaches gemm.hip only through an epilogue gemm.hip has itself for
    that layout (bias + GELU with a K-inner B; its GELU' form wants a K-outer B, hence N % 256 == 0):
    the plain store of that width goes to gemm_small's narrower tiles."""
    if N % 256 == 0:
        return "gemm8"
    if N <= 192 and not own_epilogue:
        return "gemm_small"
    return "gemm" if k_inner_b else "gemm_small"


def check_fused(O, cuda, shapes):
    for (M, N, K) in shapes:
        # tilt: sums spread over +-24 K grid units (H needs rounding; gelu saturated);
        # without: |h| of a few units, the range where gelu_new and gelu_new' are not linear
        for tilt in (True, False):
            for trans_w in (False, True):
                tag = f"{(M, N, K)} tilt={tilt} trans_w={trans_w}"
                # forward: h = bf16(x W^T + bias); w is W [N, K] or, with trans_w, W^T [K, N]
                p = gc.exact_problem(M, N, K, seed=1, a_max=8 if tilt else 3, bias=True, tilt=tilt, device=cuda)
                w = p.b.t().contiguous() if trans_w else p.b
                ref = p.ref64()
                with gc.took(f"gemm_gelu {tag}", **{_fused_backend(N, not trans_w): 1}):
                    H, G = O.gemm_gelu(p.a, w, p.bias, trans_w)
                gc.expect_exact(H, ref, f"gemm_gelu H {tag}", tile=gc.TILE)
                gc.expect_ulp(G, gc.gelu_new64(H), f"gemm_gelu G {tag}")
                with gc.took(f"gemm_gelu_d {tag}", **{_fused_backend(N, not trans_w, False): 1}):
                    D, G = O.gemm_gelu_d(p.a, w, p.bias, trans_w)
                h = ref.float().bfloat16()
                gc.expect_ulp(G, gc.gelu_new64(h), f"gemm_gelu_d G {tag}")
                gc.expect_ulp(D, gc.gelu_new_grad64(h), f"gemm_gelu_d D {tag}")

                # backward: dg = bf16(dy W); w is W [K, N] or, with trans_w, W^T [N, K]
                q = gc.exact_problem(M, N, K, seed=2, a_max=8 if tilt else 3, tilt=tilt, device=cuda)
                w = q.b if trans_w else q.b.t().contiguous()
                dg = q.ref64().float().bfloat16().double()
                pre = gc.grid_values((N,), 8, seed=3, grid=1.0, dtype=torch.float32, device=cuda)
                F = gc.grid_values((M, N), 16, seed=4, device=cuda)
                dbias = pre.clone()
                with gc.took(f"gemm_dgelu {tag}", **{_fused_backend(N, trans_w, False): 1}):
                    C = O.gemm_dgelu(q.a, w, F, dbias, trans_w)
                gc.expect_ulp(C, dg * gc.gelu_new_grad64(F), f"gemm_dgelu C {tag}")
                gc.expect_colsum(dbias, pre, C, f"gemm_dgelu dbias {tag}")
                Dm = gc.grid_values((M, N), 6, seed=5, device=cuda)
                dbias = pre.clone()
                with gc.took(f"gemm_dmul {tag}", **{_fused_backend(N, trans_w, False): 1}):
                    C = O.gemm_dmul(q.a, w, Dm, dbias, trans_w)
                gc.expect_exact(C, dg * Dm.double(), f"gemm_dmul C {tag}", tile=gc.TILE)
                gc.expect_colsum(dbias, pre, C, f"gemm_dmul dbias {tag}")


def test_gemm8_fused_epilogues(cuda, O):
    check_fused(O, cuda, gc.FUSED_SHAPES)


def test_fused_ops_outside_gemm8_contract(cuda, O):
    """N = 384: gemm.hip or the unfused pair (store + gelu_fwd / gelu_fwd_d / gelu_bwd_colsum /
    mul_colsum); the column-sum kernels on a row tail and a partial 512-column block"""
    check_fused(O, cuda, gc.FUSED_N384_SHAPES)


def test_fused_ops_on_a_narrow_output(cuda, O):
    """N = 128, K = 64: gemm8 refuses all four; gemm.hip fuses bias + GELU for a K-inner weight; every
    other form is the unfused pair, whose store goes to gemm_small (N <= 192)"""
    check_fused(O, cuda, gc.FUSED_NARROW_SHAPES)


# ------------------------------------------------------------------------------------------------ weight gradients
def _guarded(p, cuda):
    """c as a row slice of a larger buffer: 8 sentinel rows before and after it"""
    M, N, _ = p.shape
    big = torch.full((M + 16, N), SENTINEL, device=cuda)
    c = big[8:8 + M]
    c.copy_(p.c)
    return big, c


def _guards_intact(big, what):
    assert bool((big[:8] == SENTINEL).all()) and bool((big[-8:] == SENTINEL).all()), f"{what}: guard rows written"


def test_gemm8_weight_gradients(cuda, O):
    for (T, M, N, S) in gc.WGRAD_TN:
        what = f"gemm_acc_f32 TN tokens={T} c={(M, N)} (S={S})"
        p = gc.exact_problem(M, N, T, a_max=3, c=True, device=cuda)
        big, c = _guarded(p, cuda)
        with gc.took(what, gemm8=1):
            O.gemm_acc_f32(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False)
        gc.expect_exact(c, p.ref64(), what, tile=gc.TILE)
        _guards_intact(big, what)
    M, N, K = gc.WGRAD_NT
    p = gc.exact_problem(M, N, K, c=True, device=cuda)
    big, c = _guarded(p, cuda)
    with gc.took("gemm_acc_f32 NT", gemm8=1):
        O.gemm_acc_f32(p.a, p.b, c, False, True)
    gc.expect_exact(c, p.ref64(), "gemm_acc_f32 NT", tile=gc.TILE)
    _guards_intact(big, "gemm_acc_f32 NT")


def test_gemm8_shared_weight_gradient_series(cuda, O):
    """first / middle / last on persistent slabs, twice on the same c: c is untouched until `last`, then
    start + the sum of the three products, exactly; the second series' `first` resets the slabs"""
    M, N, T = gc.SHARED_SHAPE
    try:
        start = gc.exact_problem(M, N, T, a_max=3, c=True, device=cuda).c
        c = start.clone()
        want = start.double()
        for series in range(2):
            for i in range(3):
                p = gc.exact_problem(M, N, T, seed=10 + 3 * series + i, a_max=3, device=cuda)
                before = c.clone()
                with gc.took(f"gemm_acc_f32_shared series {series} call {i}", gemm8=1):
                    O.gemm_acc_f32_shared(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False, i == 0, i == 2)
                want = want + p.ref64()
                if i < 2:
                    assert torch.equal(c, before), f"series {series}: c written before the last call"
            assert float(want.abs().max()) / gc.GRID < 2.0 ** 24
            gc.expect_exact(c, want, f"gemm_acc_f32_shared series {series}", tile=gc.TILE)
    finally:
        torch.ops.dedloc_ws.clear_workspaces()


# (M, N, K) of c [M, N] += over K tokens -> the split count of gemm8's weight gradient on 256 CUs
WGRAD_SPLITS = {(3072, 1024, 262144): 16, (1024, 1024, 262144): 16, (4096, 1024, 262144): 4, (1024, 4096, 262144): 4,
                (256, 256, 25088): 49, (512, 512, 25088): 49, (2048, 512, 25088): 14, (256, 256, 3136): 7,
                (768, 256, 1024): 4, (256, 256, 512): 2, (256, 256, 256): 1, (256, 256, 64): 1,
                (256, 256, 100): 1}  # the last: K no multiple of 64


def test_gemm_wgrad_split_table(O):
    """host arithmetic only (nothing is launched): the split choice stays what it was"""
    got = {s: int(torch.ops.dedloc_ws.gemm_wgrad_splits(*s)) for s in WGRAD_SPLITS}
    assert got == WGRAD_SPLITS


# ------------------------------------------------------------------------------------------------ gemm.hip
def test_gemm_tiled_store(cuda, O):
    """N = 384 / 640 (a partial last column tile), M = 256 / 300, nk = 1 / 3; the LDS-staged 16-byte
    store path (no residual) and the per-element one (residual)"""
    check_store(O, cuda, gc.TILED_SHAPES, ("NT",), "gemm")


def test_gemm_tiled_split_k_covers_every_row(cuda, O):
    """One 256 x 256 tile over 66624 reduction rows into a non-contiguous c (gemm8 declines): the
    dispatch asks gemm.hip for 65 splits, and 66624 / 65 = 1024 rows each used to leave rows
    66560..66623 unread.  Data in {-1, 0, 1}."""
    M, N, K = gc.SPLIT_DEFECT
    p = gc.exact_problem(M, N, K, a_max=1, b_max=1, grid=1.0, c=True, tilt=False, device=cuda)
    big = torch.full((M, 2 * N), SENTINEL, device=cuda)
    c = big[:, :N]
    c.copy_(p.c)
    dy, x = p.a.t().contiguous(), p.b.t().contiguous()
    with gc.took("gemm_acc_f32 into a column slice", gemm=1):
        O.gemm_acc_f32(dy, x, c, True, False)
    gc.expect_exact(c, p.ref64(), "gemm_acc_f32 K=66624 on gemm.hip", tile=gc.TILE)
    assert bool((big[:, N:] == SENTINEL).all()), "the other half of the buffer was written"


# ------------------------------------------------------------------------------------------------ gemm_small
def test_gemm_small_store(cuda, O):
    check_store(O, cuda, gc.SMALL_SHAPES, ("NT", "NN", "TN"), "gemm_small")


def test_gemm_small_split_reduction(cuda, O):
    """2 and 4 fp32 slabs, finished (bias, residual, one rounding) by slab_finish_kernel"""
    check_store(O, cuda, tuple(s[:3] for s in gc.SMALL_SPLIT_SHAPES), ("NT", "NN"), "gemm_small")


def test_gemm_small_column_slices(cuda, O):
    """operands as column slices of wider tensors at element offsets 0 (16-byte aligned: the vector
    walk) and 3 (the element-wise walk)"""
    M, N, K = 37, 70, 96
    for off_a in (0, 3):
        for off_b in (0, 3):
            for form in ("NT", "NN"):
                what = f"gemm {form} slices at {off_a}, {off_b}"
                p = gc.exact_problem(M, N, K, seed=off_a * 4 + off_b, bias=True, residual=True, device=cuda)
                wa = torch.full((M, K + 8), 7.0, device=cuda, dtype=torch.bfloat16)
                a = wa[:, off_a:off_a + K]
                a.copy_(p.a)
                bt = p.b if form == "NT" else p.b.t()
                wb = torch.full((bt.shape[0], bt.shape[1] + 8), 7.0, device=cuda, dtype=torch.bfloat16)
                b = wb[:, off_b:off_b + bt.shape[1]]
                b.copy_(bt)
                with gc.took(what, gemm_small=1):
                    out = O.gemm(a, b, p.bias, p.res, False, form == "NT", 0)
                gc.expect_exact(out, p.ref64(), what)


def test_gemm_small_acc_f32(cuda, O):
    M, N, K = 37, 70, 96
    p = gc.exact_problem(M, N, K, c=True, device=cuda)
    for form in ("TN", "NT"):
        big, c = _guarded(p, cuda)
        with gc.took(f"gemm_acc_f32 {form}", gemm_small=1):
            if form == "TN":
                O.gemm_acc_f32(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False)
            else:
                O.gemm_acc_f32(p.a, p.b, c, False, True)
        gc.expect_exact(c, p.ref64(), f"gemm_acc_f32 {form} on gemm_small")
        _guards_intact(big, f"gemm_acc_f32 {form} on gemm_small")


def test_gemm_small_bmm(cuda, O):
    """contiguous operands, transposed views, and a batch stride that is no multiple of 8 elements"""
    for (Bn, M, N, K) in gc.BMM_SHAPES:
        probs = [gc.exact_problem(M, N, K, seed=20 + i, device=cuda) for i in range(Bn)]
        ref = torch.stack([p.ref64() for p in probs])
        a = torch.stack([p.a for p in probs])                 # [B, M, K]
        b = torch.stack([p.b.t() for p in probs]).contiguous()  # [B, K, N]
        a_t = torch.stack([p.a.t() for p in probs]).contiguous().transpose(1, 2)  # stored [B, K, M]
        b_t = torch.stack([p.b for p in probs]).transpose(1, 2)                   # stored [B, N, K]
        wide_a = torch.full((Bn, M * K + 3), 7.0, device=cuda, dtype=torch.bfloat16)
        a_s = wide_a[:, :M * K].view(Bn, M, K)
        a_s.copy_(a)
        wide_b = torch.full((Bn, K * N + 5), 7.0, device=cuda, dtype=torch.bfloat16)
        b_s = wide_b[:, :K * N].view(Bn, K, N)
        b_s.copy_(b)
        assert a_s.stride(0) % 8 and b_s.stride(0) % 8
        for name, (x, y) in {"contiguous": (a, b), "transposed": (a_t, b_t), "odd batch stride": (a_s, b_s)}.items():
            for out_f32 in (False, True):
                what = f"bmm {(Bn, M, N, K)} {name} out_f32={out_f32}"
                with gc.took(what, gemm_small=1):
                    out = O.bmm(x, y, out_f32)
                assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
                gc.expect_exact(out, ref, what)


# ------------------------------------------------------------------------------------------------ randn data
def _randn_problem(M, N, K, cuda, seed, c=False):
    g = torch.Generator().manual_seed(seed)
    p = gc.Exact(torch.randn(M, K, generator=g).bfloat16().to(cuda), torch.randn(N, K, generator=g).bfloat16().to(cuda),
                 bias=torch.randn(N, generator=g).to(cuda), res=torch.randn(M, N, generator=g).bfloat16().to(cuda))
    if c:
        p.bias = p.res = None
        p.c = torch.randn(M, N, generator=g).to(cuda)
    return p


def _bounded_store(O, cuda, shape, form, backend, seed):
    M, N, K = shape
    p = _randn_problem(M, N, K, cuda, seed)
    what = f"{backend} gemm {form} {shape}"
    with gc.took(what, **{backend: 1}):
        out = store(O, p, form)
    gc.expect_bounded(out, p.ref64(), p.abs_ab(), K, True, p.extras(), what, kernel=backend)


def test_gemm8_bounded_on_randn(cuda, O):
    """(300, 512, 320) NT and NN; the TN form (both operands K-outer) exists in gemm8 only for the fp32
    weight gradient and needs M % 256 == 0, so it runs at (256, 512, 320) through gemm_acc_f32, and
    `gemm` TN at (300, 512, 320) is held to the same bound on the kernel that takes it (gemm_small)."""
    _bounded_store(O, cuda, (300, 512, 320), "NT", "gemm8", 1)
    _bounded_store(O, cuda, (300, 512, 320), "NN", "gemm8", 2)
    _bounded_store(O, cuda, (300, 512, 320), "TN", "gemm_small", 3)
    p = _randn_problem(256, 512, 320, cuda, 4, c=True)
    c = p.c.clone()
    with gc.took("gemm8 gemm_acc_f32 TN", gemm8=1):
        O.gemm_acc_f32(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False)
    gc.expect_bounded(c, p.ref64(), p.abs_ab(), 320, False, p.extras(), "gemm8 gemm_acc_f32 TN (256, 512, 320)",
                      kernel="gemm8")


def test_gemm_tiled_bounded_on_randn(cuda, O):
    _bounded_store(O, cuda, (300, 384, 192), "NT", "gemm", 5)


def test_gemm_small_bounded_on_randn(cuda, O):
    _bounded_store(O, cuda, (37, 70, 1100), "NT", "gemm_small", 6)


# ------------------------------------------------------------------------------------------------ property
hypothesis = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

FUZZ = settings(max_examples=12, deadline=None, derandomize=True,
                suppress_health_check=[HealthCheck.function_scoped_fixture])


@FUZZ
@given(M=st.integers(1, 1100), N=st.sampled_from([256, 512, 768]), kt=st.integers(1, 6), bias=st.booleans(),
       residual=st.booleans(), form=st.sampled_from(["NT", "NN"]), seed=st.integers(0, 2**16))
def test_gemm8_store_property(cuda, O, M, N, kt, bias, residual, form, seed):
    K = 64 * kt
    what = f"gemm {form} {(M, N, K)} bias={bias} residual={residual} seed={seed}"
    p = gc.exact_problem(M, N, K, seed=seed, bias=bias, residual=residual, device=cuda)
    ref = p.ref64()
    with gc.took(what, gemm8=1):
        out = store(O, p, form)
    gc.expect_exact(out, ref, what, tile=gc.TILE)
