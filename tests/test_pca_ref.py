"""CPU: the inputs of the seqFitPCA tests are fit for their bounds -- for every driver case of pca_ref.py the numpy
restatement of the iteration converges to tol within max_iter, and the gap below the last wanted eigenvalue of the
long-double K exceeds 1e-3 of the largest -- and the restatement itself agrees with numpy.linalg.eigh."""
import numpy as np
import pytest

import pca_ref as P

from saigegds_amd import seqFitPCA


@pytest.mark.parametrize("c", P.DRIVER_CASES, ids=P.case_id)
def test_driver_case_converges_and_has_a_gap(c):
    n, m, p = c
    n_pc = p - 1
    codes = P.structured_codes(n, m, p)
    res = seqFitPCA(P.source(codes), n_pc=n_pc, n_extra=P.N_EXTRA, tol=P.TOL, max_iter=P.MAX_ITER, verbose=False,
                    operator_factory=P.NumpyPcaGrm, **P.FILTER)
    assert res["snp.id"].size == m                      # every generated marker passes the filter: K is dense_K's
    assert res["converged"].all() and res["n.iter"] <= P.MAX_ITER
    assert (res["resid"] <= P.TOL * res["eigenval"][0]).all()
    K, lam = P.dense_K(n, m, p)
    gap = lam[n_pc - 1] - lam[n_pc]
    print(f"\n{P.case_id(c)}: rounds {res['n.iter']}, lambda {lam[:n_pc + 1]}, gap / lambda_1 = {gap / lam[0]:.3g}")
    assert gap > 1e-3 * lam[0]
    np.testing.assert_allclose(res["eigenval"], lam[:n_pc], rtol=0, atol=res["resid"].max() + 1e-9 * lam[0])


def test_restatement_matches_eigh_on_a_small_matrix():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((40, 60))
    K = A @ A.T / 60 + np.diag(np.r_[30.0, 20.0, 10.0, np.zeros(37)])
    r = P.subspace_pca(K, 3, rng.standard_normal((9, 40)), max_iter=200, tol=1e-10)
    lam, V = np.linalg.eigh(K)
    assert r["n_converged"] == 3
    np.testing.assert_allclose(r["eigval"], lam[::-1][:3], rtol=1e-9)
    for c in range(3):
        assert P.sine(r["vec"][c], V[:, -1 - c]) <= 1e-7
        assert r["vec"][c][np.argmax(np.abs(r["vec"][c]))] > 0


def test_rank_breakdown_is_reported():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((30, 5))
    with pytest.raises(P.PcaRankError):
        P.subspace_pca(A @ A.T, 8, rng.standard_normal((12, 30)), max_iter=10)
