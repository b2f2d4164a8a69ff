"""The row-kernel checker (tests/row_checks.py) against the CPU implementations of the same operators:
every case of the GPU tier (tests/test_row_kernels_exact_gpu.py) passes on them — so the generators
keep their promises (sums exact in fp32, bounds reachable) and the CPU reference is held to the same
assertions as the kernels — and each check catches a planted localized defect that the older
whole-tensor ``rel < 1e-2`` cannot see."""
import pytest
import torch

import dedloc_amd.ops  # noqa: F401
import row_checks as rc

O = torch.ops.dedloc
CPU = "cpu"


# ------------------------------------------------------------------------------------------------ every GPU-tier case
@pytest.mark.parametrize("D", rc.LN_D)
def test_layernorm_fwd_cases(D):
    for rows in rc.LN_FWD_ROWS:
        for with_res in (False, True):
            rc.run_ln_fwd(O, rows, D, with_res, CPU)
            rc.run_ln_fwd(O, rows, D, with_res, CPU, integer=True)


def _ln_bwd_variants(rows, D, device):
    for accumulate in (False, True):
        for with_dsum in (False, True):
            rc.run_ln_bwd(O, rows, D, accumulate, with_dsum, device)
        rc.run_ln_bwd(O, rows, D, accumulate, False, device, integer=True)


@pytest.mark.parametrize("D", rc.LN_D)
def test_layernorm_bwd_cases(D):
    for rows in rc.LN_BWD_ROWS:
        _ln_bwd_variants(rows, D, CPU)


@pytest.mark.parametrize("rows,D", rc.LN_BWD_BIG)
def test_layernorm_bwd_big_cases(rows, D):
    _ln_bwd_variants(rows, D, CPU)


def test_gelu_cases():
    for n in rc.GELU_N:
        rc.run_gelu_fwd(O, n, CPU)
    for n in rc.GELU_BWD_N:
        rc.run_gelu_bwd(O, n, CPU)


def test_colsum_cases():
    for rows in rc.COLSUM_ROWS:
        for N in rc.COLSUM_N:
            rc.run_gelu_bwd_dbias(O, rows, N, CPU)
            for acc in (False, True):
                rc.run_bias_grad(O, rows, N, acc, CPU)
    for rows in rc.COLSUM_SCALAR_ROWS:
        for N in rc.COLSUM_SCALAR_N:
            for acc in (False, True):
                rc.run_bias_grad(O, rows, N, acc, CPU)


def test_tanh_and_cast_cases():
    for n in rc.TANH_N:
        rc.run_tanh(O, n, CPU)
    for n in rc.CAST_N:
        rc.run_cast(O, n, CPU)


@pytest.mark.parametrize("E", rc.EMBED_E)
def test_embedding_cases(E):
    for (B, S) in rc.EMBED_BS:
        for tt_mode in rc.EMBED_TT:
            q = rc.embed_problem(E, B, S, tt_mode)
            what = f"embed E={E} B={B} S={S} tt={tt_mode}"
            rc.run_embed_fwd(O, q, what)
            rc.run_embed_bwd(O, q, what)
    B, S, hot = rc.EMBED_HOT
    q = rc.embed_problem(E, B, S, "two", hot=hot)
    assert int((q["ids"] == 7).sum()) >= hot
    rc.run_embed_fwd(O, q, f"embed E={E} hot id")
    rc.run_embed_bwd(O, q, f"embed E={E} hot id")
    for T in rc.EMBED_PACKED_T:
        for tt_mode in rc.EMBED_TT:
            q = rc.embed_problem(E, 1, T, tt_mode, packed=True)
            rc.run_embed_fwd(O, q, f"embed packed E={E} T={T} tt={tt_mode}")
            rc.run_embed_bwd(O, q, f"embed packed E={E} T={T} tt={tt_mode}")


def test_embed_bwd_rejects_a_partial_sequence():
    q = rc.embed_problem(64, 3, 5, "two")
    ds = torch.zeros(15, 64, dtype=torch.bfloat16)
    grads = [torch.zeros_like(q[k]) for k in ("w", "p", "t")]
    with pytest.raises(RuntimeError, match="whole number of sequences"):
        O.embed_bwd(ds, q["ids"], q["tt"], *grads, 4)
    with pytest.raises(RuntimeError, match="ds has"):
        O.embed_bwd(ds[:10], q["ids"], q["tt"], *grads, 5)
    assert all(float(g.abs().sum()) == 0.0 for g in grads)


def test_xent_cases():
    for (M, V) in rc.XENT_SHAPES:
        for pin in (0, 1):
            rc.run_xent(O, M, V, pin, CPU)
    rc.run_xent(O, 9, 8, 0, CPU, all_ignored=True)
    rc.run_xent(O, 5, 2047, 0, CPU, all_ignored=True)


@pytest.mark.parametrize("gs", rc.OPT_GRAD_SCALES)
def test_optimizer_cases(gs):
    """On the CPU operator the bound is met by construction; what this pins is that its error against
    the fp64 replay is a rounding error (the replay is the same formula), not a formula mismatch: a few
    u for p and v (m and buf, sums of two terms that may cancel, are normalised by |ref| all the same and
    so have no such ceiling)."""
    figs = rc.run_optimizer(O, "lamb", gs, CPU)
    for clip in (False, True):
        figs += rc.run_optimizer(O, "larc", gs, CPU, clip=clip)
    worst = max(f["cpu_worst"] for f in figs if f["quantity"] in ("p", "v"))
    assert worst < 8 * rc.U, worst


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.fixture(autouse=True)
def _margins_of_the_cases_only(request, monkeypatch):
    if not request.node.name.split("[")[0].endswith("_cases"):
        monkeypatch.setattr(rc, "RECORD", False)


@pytest.fixture(scope="module")
def ln1000():
    """A correct LayerNorm forward and backward at rows = 1000, D = 768 (the older test's row count)."""
    rows, D = 1000, 768
    x, r, gamma, beta = rc.ln_problem(rows, D, True)
    y, s, mean, rstd = O.layernorm_fwd(x, r, gamma, beta, rc.EPS)
    dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(5)).bfloat16()
    dgamma, dbeta, dsum = torch.zeros(D), torch.zeros(D), torch.zeros(D)
    ds = O.layernorm_bwd(dy, s, gamma, mean, rstd, dgamma, dbeta, False, dsum)
    zero = torch.zeros(D)
    rc.check_ln_fwd_outputs(y, mean, rstd, s, gamma, beta, "good")
    rc.check_ln_bwd(ds, dgamma, dbeta, dsum, (zero, zero, zero), dy, s, gamma, mean, rstd, "good")
    return dict(y=y, s=s, mean=mean, rstd=rstd, gamma=gamma, beta=beta, dy=dy, ds=ds, dgamma=dgamma, dbeta=dbeta,
                dsum=dsum, zero=zero)


def test_flipped_ulp_in_y_caught_and_missed_by_rel(ln1000):
    """One ulp away from the reference.  2^-8 |ref| is bf16's half ulp at the bottom of a binade and a
    whole one at its top, so the element is the first of its row in the lower half of a binade."""
    L = ln1000
    _, _, xh, _ = rc.ln_stats64(L["s"])
    ref = xh * L["gamma"].double() + L["beta"].double()
    r = 999
    c = int((torch.frexp(ref[r])[0].abs() < 0.7).nonzero()[0])
    away = 1 if abs(float(L["y"][r, c])) >= abs(float(ref[r, c])) else -1
    bad = L["y"].clone()
    bad.view(torch.int16)[r, c] += away
    assert rc.rel(bad, L["y"]) < 1e-2
    with pytest.raises(AssertionError, match=rf"1 of 768000 elements outside the bound.*row {r}, column {c}"):
        rc.check_ln_fwd_outputs(bad, L["mean"], L["rstd"], L["s"], L["gamma"], L["beta"], "planted")


def test_zeroed_chunk_in_ds_caught_and_missed_by_rel(ln1000):
    L = ln1000
    bad = rc.zero_chunk(L["ds"], 517, 33)
    assert not torch.equal(bad, L["ds"]) and rc.rel(bad, L["ds"]) < 1e-2
    with pytest.raises(AssertionError, match=r"planted ds: \d of 768000 elements outside the bound.*row 517, column 26[4-9]"):
        rc.check_ln_bwd(bad, L["dgamma"], L["dbeta"], L["dsum"], (L["zero"],) * 3, L["dy"], L["s"], L["gamma"], L["mean"],
                        L["rstd"], "planted")


def test_duplicated_last_row_caught_and_missed_by_rel(ln1000):
    """One wrong row of ``rows`` independent ones moves ``rel`` by about sqrt(2 / rows): 4.5 % at 1000 rows,
    where the old metric does see it, under 1 % at 32768 (the workload has 262144).  So the miss is
    asserted on a 32768-row output, the catch on both."""
    L = ln1000
    with pytest.raises(AssertionError, match="row 999"):
        rc.check_ln_fwd_outputs(rc.duplicate_last_row(L["y"]), L["mean"], L["rstd"], L["s"], L["gamma"], L["beta"], "planted")
    x, _, gamma, beta = rc.ln_problem(32768, 64, False)
    y, s, mean, rstd = O.layernorm_fwd(x, None, gamma, beta, rc.EPS)
    bad = rc.duplicate_last_row(y)
    assert not torch.equal(bad, y) and rc.rel(bad, y) < 1e-2
    with pytest.raises(AssertionError, match="row 32767"):
        rc.check_ln_fwd_outputs(bad, mean, rstd, s, gamma, beta, "planted")


def test_neighbours_mean_caught_and_missed_by_rel():
    x, _, gamma, beta = rc.ln_problem(32768, 64, False, integer=True)
    y, s, mean, rstd = O.layernorm_fwd(x, None, gamma, beta, rc.EPS)
    i = next(i for i in range(1000, 32768) if mean[i] != mean[i - 1])
    bad = rc.swap_in_neighbour(mean, i)
    assert rc.rel(bad, mean) < 1e-2
    with pytest.raises(AssertionError, match=rf"planted mean: 1 of 32768 elements outside the bound.*row {i}, column 0"):
        rc.check_ln_fwd_outputs(y, bad, rstd, s, gamma, beta, "planted")


def test_dropped_term_of_a_column_sum_caught_and_missed_by_rel(ln1000):
    g = torch.Generator().manual_seed(6)
    dy = rc.ints(g, (200, 257))
    before = rc.nonzero_ints(g, (257,))
    dbias = before.clone()
    O.bias_grad(dy, dbias, True)
    r, c = next((r, 256) for r in range(199, -1, -1) if dy[r, 256] != 0)
    bad = rc.drop_one_term(dbias, dy, r, c)
    assert rc.rel(bad, dbias) < 1e-2
    with pytest.raises(AssertionError, match="1 of 257 elements differ"):
        rc.expect_colsum_exact(bad, before, dy, "planted")
    # the bounded form of the check (LayerNorm's dgamma over real-valued rows)
    L = ln1000
    xh = (L["s"].float() - L["mean"][:, None]) * L["rstd"][:, None]
    bad = L["dgamma"].clone()
    bad[700] -= L["dy"][999, 700].float() * xh[999, 700]
    assert bad[700] != L["dgamma"][700] and rc.rel(bad, L["dgamma"]) < 1e-2
    with pytest.raises(AssertionError, match=r"planted dgamma: 1 of 768 elements outside the bound.*column 700"):
        rc.check_ln_bwd(L["ds"], bad, L["dbeta"], L["dsum"], (L["zero"],) * 3, L["dy"], L["s"], L["gamma"], L["mean"],
                        L["rstd"], "planted")


def test_id_added_twice_caught_and_missed_by_rel():
    """16384 tokens: one token's share of ``rel`` is about 1 / sqrt(tokens); the sums stay below 2^24."""
    q = rc.embed_problem(64, 128, 128, "two")
    grads, before, ds = rc.run_embed_bwd(O, q, "good")
    token = next(t for t in range(16383, -1, -1) if float(ds[t].float().abs().sum()) > 0)
    bad = rc.add_id_twice(grads[0], ds, q["ids"], token)
    assert not torch.equal(bad, grads[0]) and rc.rel(bad, grads[0]) < 1e-2
    with pytest.raises(AssertionError, match=rf"planted dwemb: \d+ of {rc.EMBED_VOCAB * 64} elements differ; first \(row, col, "
                                             rf"got, want\): \[\({int(q['ids'][token])}, "):
        rc.check_embed_bwd([bad, grads[1], grads[2]], before, ds, q, "planted")


def test_shifted_label_column_caught_and_missed_by_rel():
    M, V = 32768, 8
    x, lab = rc.xent_problem(M, V)
    loss, grad = O.xent_fwd_bwd(x, lab, False, rc.IGNORE)
    rc.check_xent(loss, grad, x, lab, "good")
    row = next(r for r in range(M - 1, -1, -1) if lab[r] > 0)
    bad = rc.shift_label_column(grad, lab, row, 1.0 / (M - 1))
    assert rc.rel(bad, grad) < 1e-2
    with pytest.raises(AssertionError, match=rf"planted grad: 2 of {M * V} elements outside the bound.*row {row}, column "
                                             rf"{int(lab[row]) - 1}"):
        rc.check_xent(loss, bad, x, lab, "planted")


def test_nan_is_caught():
    """An error comparison alone passes NaN (NaN > bound is false): every check tests for it."""
    h = rc.activations(torch.Generator().manual_seed(7), (64,))
    y = O.gelu_fwd(h)
    y[63] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        rc.expect_finite_ulp(y, rc.gelu_new64(h), "planted")
    with pytest.raises(AssertionError, match="outside the bound"):
        rc.expect_within(y.float(), rc.gelu_new64(h), 1.0, "planted", record=False)
