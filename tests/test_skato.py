"""SKAT-O on the host: the vectorised mixture tail against the scalar one, the closed forms of B_rho and
W, the grid of one value against the SKAT driver's own p-value and the burden chi-square, the bounds, the combined
p-value against a Monte Carlo count (tests/skato_ref.py), and the driver ``seqAssocGLMM_spaSKATO`` with the injected
reference scanner of tests/test_skat.py -- which has no ``skato_spectra``, so every spectrum here is numpy's."""
import math

import numpy as np
import pytest

import skato_ref as R
from test_skat import driver_case, lambda_sets, ref_scanner_factory

# The Monte Carlo acceptance: |pval - MC| <= 4 standard errors + MARGIN * MC.  MARGIN is twice the worst relative gap
# measured on the four cases below (8.2 % at m = 12, T = 0.01; 6.8 %, 0.2 % and 0.04 % on the others).
# The gap is the method's own approximation: the saddlepoint tail (2.5 - 8 % off a Monte Carlo count at p = 0.01 on these
# spectra), the quadrature across the kink of delta(x), and the remainder taken as independent of the burden direction.
# That last one is exact only where the cross term vz vanishes, so the cases (unit variances, correlation 0.3 inside
# the block) keep vz under 5 % of the remainder's variance vQ: the test is to catch a wrong implementation, and a
# block of correlation 0.5 on half the variants (vz / vQ = 0.11 - 0.20) moves the METHOD by 11 - 19 %, which a count with
# the remainder's draws shuffled against the burden's reproduces.
MARGIN = 0.164
MC_CASES = [(5, 3, 0.01), (5, 3, 0.7), (12, 4, 0.01), (12, 4, 0.7)]


@pytest.mark.parametrize("name", ["equal", "geometric", "dominant", "golden Phi"])
def test_vectorised_tail_equals_the_scalar_function(name):
    from saigegds_amd.skat import pchisq_mix
    from saigegds_amd.skato import pchisq_mix_vec
    lam = lambda_sets()[name]
    mean, sd = float(lam.sum()), math.sqrt(2 * float(np.sum(lam * lam)))
    q = np.concatenate([np.linspace(mean - 3 * sd, mean + 12 * sd, 257), mean * np.logspace(-6, 2, 64),
                        [mean, 0.0, -1.0, float("nan"), float("inf")]])
    got = pchisq_mix_vec(q, lam)
    ref = np.array([pchisq_mix(float(x), lam) for x in q])
    assert got.shape == q.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    k = ~np.isnan(ref)
    rel = np.abs(got[k] - ref[k]) / ref[k]
    print(name, "worst relative difference", rel.max(), "bit-equal", int(np.sum(got[k] == ref[k])), "of", int(k.sum()))
    assert np.all(rel <= 1e-13)
    assert np.all(np.isnan(pchisq_mix_vec([1.0, 2.0], []))) and pchisq_mix_vec(np.zeros((2, 0)), lam).shape == (2, 0)
    one = pchisq_mix_vec(q, [2.5, 1e-11])
    assert np.array_equal(one[k], [pchisq_mix(float(x), [2.5]) for x in q[k]])


@pytest.mark.parametrize("m", [1, 2, 5, 12, 33])
def test_closed_forms(m):
    from saigegds_amd.skato import skato_matrices
    A = R.block_case(m, (m + 1) // 2, 100 + m)
    grid = R.RHO
    mats = skato_matrices(A, grid)
    assert len(mats) == len(grid) + 1 and np.array_equal(mats[0], A)                 # rho = 0: A's own bits
    scale = float(np.abs(A).sum())
    for B, rk in zip(mats, R.capped(grid)):
        ref = R.b_rho_plain(A, rk)
        assert np.array_equal(B, B.T)
        assert np.max(np.abs(B - ref)) <= 64 * np.finfo(float).eps * scale, (m, rk)
    W = mats[-1]
    assert np.max(np.abs(W @ np.ones(m))) <= 16 * m * np.finfo(float).eps * scale
    assert np.max(np.abs(W - W.T)) <= 4 * np.finfo(float).eps * scale
    # a grid of one value is taken as it is: rho = 1 is not capped, B_1 = (c / m) 11'
    B1 = skato_matrices(A, (1,))[0]
    assert np.max(np.abs(B1 - A.sum() / m)) <= 64 * np.finfo(float).eps * scale


def _s_for(A, target, seed):
    """A score vector whose observed T = min_rho p_rho is near ``target``: a fixed direction, scaled by bisection."""
    from saigegds_amd.skat import pchisq_mix
    from saigegds_amd.skato import skato_matrices
    lams = [np.linalg.eigvalsh(B) for B in skato_matrices(A, R.RHO)[:-1]]
    re = R.capped(R.RHO)
    d = np.linalg.cholesky(A) @ np.random.default_rng(seed).standard_normal(A.shape[0])
    T = lambda f: min(pchisq_mix(float((1 - rk) * np.sum((f * d) ** 2) + rk * np.sum(f * d) ** 2), lam)   # noqa: E731
                      for rk, lam in zip(re, lams))
    lo, hi = 1e-3, 1e3
    for _ in range(60):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if T(mid) > target else (lo, mid)
    return math.sqrt(lo * hi) * d


@pytest.mark.parametrize("m,n_block,target", MC_CASES)
def test_pvalue_against_monte_carlo(m, n_block, target):
    from saigegds_amd.skato import skato_pvalue
    A = R.block_case(m, n_block, 0, corr=0.3)
    s = _s_for(A, target, 7 * m)
    res = skato_pvalue(s, A, R.RHO)
    T = res["T"]
    assert abs(T - target) <= 1e-6 * target
    mc, se = R.monte_carlo(A, T)
    gap = abs(res["pval"] - mc)
    print(f"m = {m}, T = {T:.6g}: pval {res['pval']:.6g}, Monte Carlo {mc:.6g} +- {se:.2g}, relative gap {gap / mc:.4f}, "
          f"rho.min {res['rho.min']}")
    assert T <= res["pval"] <= min(1.0, len(R.RHO) * T)
    assert gap <= 4 * se + MARGIN * mc


@pytest.mark.parametrize("m", [1, 2, 5, 12, 40])
def test_grid_of_one_value_and_bounds(m):
    from scipy.special import chdtrc
    from saigegds_amd.skat import pchisq_mix
    from saigegds_amd.skato import skato_pvalue
    A = R.block_case(m, (m + 1) // 2, 300 + m)
    rng = np.random.default_rng(m)
    for scale in (0.2, 1.0, 2.5):
        s = scale * (np.linalg.cholesky(A) @ rng.standard_normal(m))
        skat = pchisq_mix(float(np.sum(s * s)), np.linalg.eigvalsh(A))          # what the SKAT driver computes
        r0 = skato_pvalue(s, A, (0,))
        assert r0["pval"] == skat and r0["p.SKAT"] == skat and r0["T"] == skat and r0["rho.min"] == 0.0
        burden = float(chdtrc(1.0, float(np.sum(s)) ** 2 / float(A.sum(axis=1).sum())))
        r1 = skato_pvalue(s, A, (1,))
        assert r1["p.burden"] == burden and r1["p.SKAT"] == skat
        assert r1["pval"] == (burden if m > 1 else skat)
        for grid in (R.RHO, (0, 1), (0.25, 0.5), (0.1,)):
            r = skato_pvalue(s, A, grid)
            assert r["p.SKAT"] == skat and r["p.burden"] == burden            # whether or not 0 and 1 are in the grid
            if m == 1:
                assert r["pval"] == skat
            else:
                assert r["T"] <= r["pval"] <= min(1.0, len(grid) * r["T"]), (m, scale, grid, r)
                assert r["rho.min"] in grid


def test_degenerate_units():
    from saigegds_amd.skato import skato_pvalue
    A = R.block_case(4, 2, 1)
    s = np.array([0.3, -1.0, 0.7, 0.2])
    assert all(math.isnan(v) for v in skato_pvalue(np.zeros(0), np.zeros((0, 0))).values())
    bad = A.copy()
    bad[1, 2] = bad[2, 1] = float("nan")
    assert math.isnan(skato_pvalue(s, bad)["pval"])
    assert math.isnan(skato_pvalue(np.array([0.3, float("inf"), 0.7, 0.2]), A)["pval"])
    # c = 1'A1 <= 0: the burden direction carries nothing, pval = p.SKAT
    neg = np.array([[1.0, -1.0], [-1.0, 1.0]])
    r = skato_pvalue(np.array([0.5, -0.2]), neg)
    assert r["pval"] == r["p.SKAT"] and math.isfinite(r["pval"]) and math.isnan(r["p.burden"])
    # A of rank one: every p_rho is the same chi-square, and so is the combination
    v = np.array([1.0, 2.0, 0.5])
    r = skato_pvalue(0.8 * v, np.outer(v, v))
    assert r["pval"] == pytest.approx(r["p.burden"], rel=1e-6) and r["T"] <= r["pval"]
    # spectra handed in (what the device returns) are used as they are
    from saigegds_amd.skato import skato_matrices
    sp = [np.linalg.eigvalsh(B) for B in skato_matrices(A, R.RHO)]
    assert skato_pvalue(s, A, R.RHO, spectra=sp) == skato_pvalue(s, A, R.RHO)


@pytest.mark.parametrize("rho", [(), (0.5, 0.25), (0, 0, 1), (-0.1, 0.5), (0, 1.5), (0, float("nan")), "a"])
def test_bad_grid(rho):
    from saigegds_amd import seqAssocGLMM_spaSKATO
    from saigegds_amd.skato import skato_pvalue
    with pytest.raises(ValueError):
        skato_pvalue(np.ones(2), np.eye(2), rho)
    src, mod, units, _ = driver_case("binary")
    with pytest.raises(ValueError):
        seqAssocGLMM_spaSKATO(src, mod, units, rho=rho, verbose=False, scanner_factory=ref_scanner_factory())


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_driver_with_reference_scanner(trait, tmp_path):
    from saigegds_amd import seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO, seqSAIGE_LoadPval
    src, mod, units, _ = driver_case(trait)
    fac = ref_scanner_factory()
    fn = str(tmp_path / "skato.RData")
    ans = seqAssocGLMM_spaSKATO(src, mod, units, verbose=False, scanner_factory=fac, res_savefn=fn)
    assert fac.calls == 1                                           # one skat_2bit call for all units
    skat = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=fac)
    names = list(ans)
    per_set = ["pval", "pval.SKAT", "pval.burden", "rho.min", "Q"]
    tail = ["n.var"] + [f"{c}.{w}" for w in ("b1_1", "b1_25") for c in per_set]
    assert names[-len(tail):] == tail and names[:len(names) - len(tail)] == list(skat)[:len(names) - len(tail)]
    assert "pval" not in ans and "n.iter" not in ans
    assert np.array_equal(ans["n.var"], skat["n.var"]) and ans["n.var"][2] == 0 and ans["n.var"][3] == 0
    for w in ("b1_1", "b1_25"):
        assert np.array_equal(ans[f"pval.SKAT.{w}"], skat[f"pval.{w}"], equal_nan=True)      # bit for bit
        assert np.array_equal(ans[f"Q.{w}"], skat[f"Q.{w}"], equal_nan=True)
        for c in per_set:
            col = ans[f"{c}.{w}"]
            assert np.isnan(col[2]) and np.isnan(col[3]) and np.isfinite(col[[0, 1, 4]]).all(), (c, w)
        p, T = ans[f"pval.{w}"][[0, 1, 4]], np.minimum(ans[f"pval.SKAT.{w}"], ans[f"pval.burden.{w}"])[[0, 1, 4]]
        assert np.all((p > 0) & (p <= 1)) and np.all(p <= 7 * T * (1 + 1e-12))
        assert np.all(np.isin(ans[f"rho.min.{w}"][[0, 1, 4]], R.RHO))
    # one weight set: no suffix; a grid of one value is the SKAT driver's p-value
    one = seqAssocGLMM_spaSKATO(src, mod, units, wbeta=[1, 25], rho=(0,), verbose=False, scanner_factory=fac)
    assert "pval" in one and "pval.b1_25" not in one
    assert np.array_equal(one["pval"], skat["pval.b1_25"], equal_nan=True)
    assert np.array_equal(one["pval.burden"], ans["pval.burden.b1_25"], equal_nan=True)
    # round trip through the result file
    back = seqSAIGE_LoadPval(fn, verbose=False)
    for c in ("n.var", "pval.b1_1", "pval.SKAT.b1_25", "pval.burden.b1_25", "rho.min.b1_1", "Q.b1_25"):
        assert np.array_equal(np.asarray(back[c], dtype=np.float64), np.asarray(ans[c], dtype=np.float64), equal_nan=True), c
