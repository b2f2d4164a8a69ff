"""Per-element and bit-exact checks of the row kernels — layernorm.hip, elementwise.hip, embedding.hip,
xent.hip, optim.hip — at every tail and variant (tests/row_checks.py: integer data whose column sums
are exact in fp32 under any atomics order, and fp64 references from the same bf16 inputs with bounds
in bf16's half ulp and u = 2^-24).  All shapes come from the tables in row_checks.py, the smallest that
reach each code path; every index is inside its table.  Each test loops over its cases: all are
sub-millisecond launches.  tests/test_row_checks_cpu.py runs the same cases on the CPU operators."""
import os
import subprocess
import sys

import pytest
import torch

import row_checks as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    import dedloc_amd.ops  # noqa: F401

    return torch.ops.dedloc


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_cases(O, cuda, Ds=rc.LN_D):
    for D in Ds:
        for rows in rc.LN_FWD_ROWS:
            for with_res in (False, True):
                rc.run_ln_fwd(O, rows, D, with_res, cuda)
                rc.run_ln_fwd(O, rows, D, with_res, cuda, integer=True)


@pytest.mark.parametrize("D", rc.LN_D)
def test_layernorm_fwd(cuda, O, D):
    """rows 1 .. 33 around the 4-wave x R-row block (R = 2 unless DEDLOC_LN_FWD_R says otherwise): y, mean,
    rstd per element, the saved sum bit for bit, the mean of integer rows exactly"""
    _ln_fwd_cases(O, cuda, (D,))


def test_layernorm_fwd_rows_per_wave_variants(cuda, O):
    """R = 1 and R = 4 rows per wave: the value is read once per process, so each runs the forward cases
    in a fresh child (which runs them directly, DEDLOC_ROW_CHECKS_CHILD set); the second child is not
    started if the first was ended by a signal or its time limit."""
    if os.environ.get("DEDLOC_ROW_CHECKS_CHILD"):
        assert os.environ.get("DEDLOC_LN_FWD_R") in ("1", "4")
        _ln_fwd_cases(O, cuda)
        return
    here = os.path.abspath(__file__)
    for R in ("1", "4"):
        env = dict(os.environ, DEDLOC_LN_FWD_R=R, DEDLOC_ROW_CHECKS_CHILD="1")
        child = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                                f"{here}::test_layernorm_fwd_rows_per_wave_variants"], env=env, timeout=120,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # a timeout raises: no second child
        assert child.returncode >= 0, f"DEDLOC_LN_FWD_R={R}: child ended by signal {-child.returncode}\n{child.stdout[-2000:]}"
        assert child.returncode == 0 and "1 passed" in child.stdout, f"DEDLOC_LN_FWD_R={R}:\n{child.stdout[-4000:]}"


def _ln_bwd_variants(O, cuda, rows, D):
    for accumulate in (False, True):
        for with_dsum in (False, True):
            rc.run_ln_bwd(O, rows, D, accumulate, with_dsum, cuda)
        rc.run_ln_bwd(O, rows, D, accumulate, False, cuda, integer=True)


@pytest.mark.parametrize("D", rc.LN_D)
def test_layernorm_bwd(cuda, O, D):
    """1, 2 and 3 blocks, a last wave iteration with one live row of two: ds per element from the mean /
    rstd passed in, dgamma / dbeta / dsum per column onto non-zero buffers, dbeta of integer rows exactly"""
    for rows in rc.LN_BWD_ROWS:
        _ln_bwd_variants(O, cuda, rows, D)


@pytest.mark.parametrize("rows,D", rc.LN_BWD_BIG)
def test_layernorm_bwd_row_ownership(cuda, O, rows, D):
    """rows = 1000: 31 blocks of 33 rows, the last with 10; rows = 1089: 34 blocks of 33, the last empty"""
    _ln_bwd_variants(O, cuda, rows, D)


# ------------------------------------------------------------------------------------------------ elementwise.hip
def test_gelu_fwd_chunk_tails(cuda, O):
    for n in rc.GELU_N:
        rc.run_gelu_fwd(O, n, cuda)


def test_gelu_bwd_tails_and_grid_cap(cuda, O):
    for n in rc.GELU_BWD_N:
        rc.run_gelu_bwd(O, n, cuda)


def test_gelu_bwd_dbias_and_bias_grad(cuda, O):
    """colsum_rows_kernel: 8 rows per wave, 64 per block, 512 columns per block, clamped tail rows"""
    for rows in rc.COLSUM_ROWS:
        for N in rc.COLSUM_N:
            rc.run_gelu_bwd_dbias(O, rows, N, cuda)
            for acc in (False, True):
                rc.run_bias_grad(O, rows, N, acc, cuda)


def test_bias_grad_scalar_path(cuda, O):
    for rows in rc.COLSUM_SCALAR_ROWS:
        for N in rc.COLSUM_SCALAR_N:
            for acc in (False, True):
                rc.run_bias_grad(O, rows, N, acc, cuda)


def test_tanh(cuda, O):
    for n in rc.TANH_N:
        rc.run_tanh(O, n, cuda)


def test_cast_bf16(cuda, O):
    for n in rc.CAST_N:
        rc.run_cast(O, n, cuda)


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("E", rc.EMBED_E)
def test_embedding(cuda, O, E):
    for (B, S) in rc.EMBED_BS:
        for tt_mode in rc.EMBED_TT:
            q = rc.embed_problem(E, B, S, tt_mode, device=cuda)
            what = f"embed E={E} B={B} S={S} tt={tt_mode}"
            rc.run_embed_fwd(O, q, what)
            rc.run_embed_bwd(O, q, what)


@pytest.mark.parametrize("E", rc.EMBED_E)
def test_embedding_hot_id(cuda, O, E):
    """300 of 512 tokens share one id: hundreds of atomics on one row of the word table"""
    B, S, hot = rc.EMBED_HOT
    q = rc.embed_problem(E, B, S, "two", hot=hot, device=cuda)
    rc.run_embed_fwd(O, q, f"embed E={E} hot id")
    rc.run_embed_bwd(O, q, f"embed E={E} hot id")


@pytest.mark.parametrize("E", rc.EMBED_E)
def test_embedding_packed(cuda, O, E):
    for T in rc.EMBED_PACKED_T:
        for tt_mode in rc.EMBED_TT:
            q = rc.embed_problem(E, 1, T, tt_mode, packed=True, device=cuda)
            rc.run_embed_fwd(O, q, f"embed packed E={E} T={T} tt={tt_mode}")
            rc.run_embed_bwd(O, q, f"embed packed E={E} T={T} tt={tt_mode}")


def test_embed_bwd_rejects_a_partial_sequence(cuda, O):
    """T % S != 0 used to run T // S sequences and drop the rest without a word"""
    q = rc.embed_problem(64, 3, 5, "two", device=cuda)
    ds = torch.zeros(15, 64, dtype=torch.bfloat16, device=cuda)
    grads = [torch.zeros_like(q[k]) for k in ("w", "p", "t")]
    with pytest.raises(RuntimeError, match="whole number of sequences"):
        O.embed_bwd(ds, q["ids"], q["tt"], *grads, 4)
    with pytest.raises(RuntimeError, match="ds has"):
        O.embed_bwd(ds[:10], q["ids"], q["tt"], *grads, 5)
    assert all(float(g.abs().sum()) == 0.0 for g in grads)


# ------------------------------------------------------------------------------------------------ cross entropy
def test_xent(cuda, O):
    """vector and scalar paths, labels pinned to columns 0 and V - 1, an ignored row, both inplace values"""
    for (M, V) in rc.XENT_SHAPES:
        for pin in (0, 1):
            rc.run_xent(O, M, V, pin, cuda)


def test_xent_all_ignored(cuda, O):
    rc.run_xent(O, 9, 8, 0, cuda, all_ignored=True)
    rc.run_xent(O, 5, 2047, 0, cuda, all_ignored=True)


# ------------------------------------------------------------------------------------------------ optimizers
@pytest.mark.parametrize("gs", rc.OPT_GRAD_SCALES)
def test_lamb(cuda, O, gs):
    """3 steps; tensors of 1 .. 4096 elements in chunks of 1000, one with zero parameters, one with a zero
    gradient (trust ratio 1); the bound of each quantity is measured on the CPU operator beside it"""
    rc.run_optimizer(O, "lamb", gs, cuda)


@pytest.mark.parametrize("gs", rc.OPT_GRAD_SCALES)
@pytest.mark.parametrize("clip", (False, True))
def test_larc_sgd(cuda, O, gs, clip):
    rc.run_optimizer(O, "larc", gs, cuda, clip=clip)
