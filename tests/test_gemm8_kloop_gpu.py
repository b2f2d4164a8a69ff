"""gemm8's K loop: the two-K-tile body with compile-time buffer parity, the scalar K advance of the
LDS-DMA sources and their 32-bit per-lane offsets (gemm8.hip).  Exact data throughout
(tests/gemm_checks.py): outputs are bit-equal to one rounding of the fp64 reference, and each call
states which kernel took it."""
import pytest
import torch

import gemm_checks as gc
from test_gemm_exact_gpu import VARIANTS, O, _guarded, _guards_intact, store  # noqa: F401  (O: fixture)

pytestmark = pytest.mark.gpu


def _splits(M, N, T):
    return int(torch.ops.dedloc_ws.gemm_wgrad_splits(M, N, T))


# ------------------------------------------------------------------------------------------------ K-tile counts
def test_gemm8_store_ktile_counts_1_to_9(cuda, O):
    """nk = 1..9: the prologue alone, the peeled tails, the leading odd K-tile, and at least two
    iterations of the two-K-tile steady body for both parities of nk; NT / NN / TN.  gemm8 has no
    bf16-store form with both operands K-outer (its only such form is the fp32 weight gradient, whose
    1..9 K-tiles test_gemm8_weight_gradient_ktiles_per_split runs): the TN store is held to the same
    exact result on whichever kernel the router gives it to, and must be exactly one launch."""
    for n in range(1, 10):
        M, N, K = 256, 256, 64 * n
        for form in ("NT", "NN", "TN"):
            for bias, residual in VARIANTS:
                what = f"gemm {form} {(M, N, K)} bias={bias} residual={residual}"
                p = gc.exact_problem(M, N, K, bias=bias, residual=residual, device=cuda)
                if form == "TN":
                    before = gc.backend_counts()
                    out = store(O, p, form)
                    got = tuple(y - x for x, y in zip(before, gc.backend_counts()))
                    assert sum(got) == 1, f"{what}: launches per kernel {dict(zip(gc.BACKENDS, got))}"
                else:
                    with gc.took(what, gemm8=1):
                        out = store(O, p, form)
                gc.expect_exact(out, p.ref64(), what, tile=gc.TILE)


# ------------------------------------------------------------------------------------------------ weight gradients
# c shapes the split table is asked about: 1 tile, 90 tiles (S = 2 beats S = 3 at 12 K-tiles), 256 tiles
# (one full wave of workgroups unsplit, so S stays 1 at 8 K-tiles)
WGRAD_C_SHAPES = ((256, 256), (2304, 2560), (4096, 4096))


def _wgrad_case(per_split, multi):
    """(M, N, T, S) with T / 64 / S == per_split K-tiles per split as the table splits it (S > 1 with
    ``multi``, else S == 1), or None when the table produces no such case on WGRAD_C_SHAPES"""
    for (M, N) in WGRAD_C_SHAPES:
        for S in (range(2, 65) if multi else (1,)):
            T = 64 * per_split * S
            if _splits(M, N, T) == S:
                return M, N, T, S
    return None


def _check_wgrad(O, cuda, M, N, T, S):
    what = f"gemm_acc_f32 TN tokens={T} c={(M, N)} (S={S}, {T // 64 // S} K-tiles per split)"
    p = gc.exact_problem(M, N, T, a_max=3, c=True, device=cuda)
    big, c = _guarded(p, cuda)
    with gc.took(what, gemm8=1):
        O.gemm_acc_f32(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False)
    gc.expect_exact(c, p.ref64(), what, tile=gc.TILE)
    _guards_intact(big, what)


def test_gemm8_weight_gradient_ktiles_per_split(cuda, O):
    """1..9 K-tiles at one split; with more than one split every count in 1..6 the table produces"""
    for n in range(1, 10):
        case = _wgrad_case(n, multi=False)
        assert case is not None, f"no unsplit weight gradient with {n} K-tiles"
        _check_wgrad(O, cuda, *case)
    # a split slice has at least 4 K-tiles (wgrad_splits8's floor): 1, 2 and 3 per split cannot occur
    cannot = (1, 2, 3)
    for n in range(1, 7):
        case = _wgrad_case(n, multi=True)
        assert (case is None) == (n in cannot), f"{n} K-tiles per split: {case}"
        if case is not None:
            _check_wgrad(O, cuda, *case)


def test_gemm8_shared_weight_gradient_odd_ktiles_per_split(cuda, O):
    """first / middle / last on persistent slabs with 5 K-tiles per split (the leading odd K-tile of
    every split, accumulate form included)"""
    M, N, T = 256, 256, 640
    S = _splits(M, N, T)
    assert S > 1 and (T // 64 // S) % 2 == 1, (S, T)
    try:
        start = gc.exact_problem(M, N, T, a_max=3, c=True, device=cuda).c
        c = start.clone()
        want = start.double()
        for i in range(3):
            p = gc.exact_problem(M, N, T, seed=20 + i, a_max=3, device=cuda)
            before = c.clone()
            with gc.took(f"gemm_acc_f32_shared call {i}", gemm8=1):
                O.gemm_acc_f32_shared(p.a.t().contiguous(), p.b.t().contiguous(), c, True, False, i == 0, i == 2)
            want = want + p.ref64()
            if i < 2:
                assert torch.equal(c, before), "c written before the last call"
        assert float(want.abs().max()) / gc.GRID < 2.0 ** 24
        gc.expect_exact(c, want, "gemm_acc_f32_shared, 5 K-tiles per split", tile=gc.TILE)
    finally:
        torch.ops.dedloc_ws.clear_workspaces()


# ------------------------------------------------------------------------------------------------ per-lane offsets
def test_gemm8_row_pitch_and_m_tail_on_a_second_column_tile(cuda, O):
    """M = 1 / 65 / 257 at N = 512, K = 192: the clamped rows of the per-lane DMA offsets, on a column
    tile whose B rows start 256 pitches into the operand"""
    for M in (1, 65, 257):
        for form in ("NT", "NN"):
            for bias, residual in VARIANTS:
                what = f"gemm {form} {(M, 512, 192)} bias={bias} residual={residual}"
                p = gc.exact_problem(M, 512, 192, bias=bias, residual=residual, device=cuda)
                with gc.took(what, gemm8=1):
                    out = store(O, p, form)
                gc.expect_exact(out, p.ref64(), what, tile=gc.TILE)


def test_gemm8_far_k_offset(cuda, O):
    """One TN weight gradient whose [T, 4096] bf16 operand is 4.03 GiB: the last K-tiles start past
    2^32 bytes, where a running 64-bit scalar base and k0 * ld must agree.  Operands are drawn on the
    GPU (the host generator of exact_problem would need tens of GiB of int64 here): integers in
    [-3, 3], the [T, 256] operand times GRID; the fp64 reference is summed over token chunks."""
    T, M, N = 528384, 4096, 256
    assert T * M * 2 > 2 ** 32 and T % 64 == 0
    a_max = 3
    # exactness precondition: every partial sum, in any order, below 2^24 grid units
    assert (a_max * gc.B_MAX * T + gc.C_MAX / gc.GRID) < 2.0 ** 24
    g = torch.Generator(device=cuda).manual_seed(7)
    a = torch.randint(-a_max, a_max + 1, (T, M), generator=g, device=cuda, dtype=torch.int8).bfloat16()
    b = (torch.randint(-gc.B_MAX, gc.B_MAX + 1, (T, N), generator=g, device=cuda, dtype=torch.int8).float()
         * gc.GRID).bfloat16()
    c0 = torch.randint(-gc.C_MAX, gc.C_MAX + 1, (M, N), generator=g, device=cuda).float()
    try:
        want = c0.double()
        chunk = 16512  # 32 chunks
        assert T % chunk == 0
        for t0 in range(0, T, chunk):
            want += a[t0:t0 + chunk].double().t() @ b[t0:t0 + chunk].double()
        assert float(want.abs().max()) / gc.GRID < 2.0 ** 24
        big = torch.full((M + 16, N), -12345.0, device=cuda)
        c = big[8:8 + M]
        c.copy_(c0)
        S = _splits(M, N, T)
        what = f"gemm_acc_f32 TN tokens={T} c={(M, N)} (S={S})"
        # the last split's last K-tile starts past 2^32 bytes of the wide operand
        assert (T - 64) * M * 2 > 2 ** 32
        with gc.took(what, gemm8=1):
            O.gemm_acc_f32(a, b, c, True, False)
        gc.expect_exact(c, want, what, tile=gc.TILE)
        _guards_intact(big, what)
    finally:
        del a, b
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ contract
def test_gemm8_refuses_a_pitch_beyond_the_lane_offsets(cuda, O):
    """A K-inner operand's tile spans 255 rows of its pitch in a 32-bit byte offset: a pitch of
    8421512 elements (255 * ld * 2 bytes > 2^32) is outside gemm8's contract and the router sends the
    call elsewhere; the same view at a pitch just inside it is gemm8's.  Checked on a strided view
    through the operator (two rows: 34 MB), not on the host function alone."""
    p = gc.exact_problem(2, 256, 64, device=cuda)
    for ld, inside in ((8421504, True), (8421512, False)):
        buf = torch.zeros(ld + 64, dtype=torch.bfloat16, device=cuda)
        a = buf.as_strided((2, 64), (ld, 1))
        a.copy_(p.a)
        before = gc.backend_counts()
        out = O.gemm(a, p.b, None, None, False, True, 0)
        got = dict(zip(gc.BACKENDS, (y - x for x, y in zip(before, gc.backend_counts()))))
        assert got["gemm8"] == (1 if inside else 0) and sum(got.values()) == 1, (ld, got)
        gc.expect_exact(out, p.ref64(), f"gemm NT with lda={ld}", tile=gc.TILE)
