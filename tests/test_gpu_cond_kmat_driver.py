"""``seqAssocGLMM_SPA_cond(grm_mat=)`` on the device: the driver's algebra on the ``Scanner``'s own
outputs, its p-values against the long-double ``Phi^K``, and the identity matrix against the closed form."""
import numpy as np
import pytest

import cond_kmat_ref as CK
import skat_kmat_ref as M
from test_cond import driver_case

pytestmark = pytest.mark.gpu
COND = [30, 77]
_runs = {}


def run(trait, which):
    """One driver call per (trait, matrix), shared by the tests: (result, the recording scanner, K, blocks, source, model)."""
    if (trait, which) not in _runs:
        import torch  # noqa: F401
        from saigegds_amd import seqAssocGLMM_SPA_cond
        from saigegds_amd._lib import Scanner
        src, mod = driver_case(trait)
        n = len(src.sample_id())
        K, blocks = (np.eye(n), [(i, i + 1) for i in range(n)]) if which == "eye" else (lambda k: (k[0], k[2]))(M.family_K(n))
        fac = CK.recording(Scanner)
        ans = seqAssocGLMM_SPA_cond(src, mod, COND, mac=4, verbose=False, scanner_factory=fac, grm_mat=(src.sample_id(), K))
        _runs[(trait, which)] = (ans, fac.last, K, blocks, src, mod)
    return _runs[(trait, which)]


def long_double(trait, which):
    """Phi^K of every kept row and of the set in long double, from the recorded call's rows and tables."""
    from saigegds_amd.cond import _tables
    from saigegds_amd.nullmod import init_nullmod
    import torch
    ans, rec, K, blocks, src, mod = run(trait, which)
    x, out8, _, _, _, _, out_c, _, _ = CK.driver_inputs(rec)
    sm = init_nullmod(mod, np.arange(len(src.sample_id())), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    idx = np.array(COND) - 1
    rows = np.concatenate([src.packed[idx], src.packed[x]])
    af = np.concatenate([out_c[:, 0], out8[x, 0]])
    lut = _tables(torch.from_numpy(af.copy()), torch.ones(af.size, dtype=torch.bool)).numpy()
    w = np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64))
    return x, CK.phi_rows(sm, rows, lut, len(COND), K, w, np.asarray(sm.tau, dtype=np.float64), "ld", blocks)


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_driver_equals_cond_tests_on_the_scanners_own_outputs(trait):
    ans, rec, *_ = run(trait, "family")
    x, beta, se, p, it = CK.driver_expected(rec, trait == "binary")
    assert int(x.sum()) == len(ans["id"]) and list(ans.keys())[-1] == "n.iter"
    for col, want in (("beta.cond", beta), ("SE.cond", se), ("pval.cond", p)):
        assert np.array_equal(ans[col], want, equal_nan=True), col
    assert np.array_equal(ans["n.iter"], it)
    ids = list(ans["id"])
    assert np.isnan(ans["pval.cond"][ids.index(30)]) and np.isnan(ans["pval.cond"][ids.index(77)])
    assert np.isfinite(np.delete(ans["pval.cond"], [ids.index(30), ids.index(77)])).all()


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_pval_against_the_long_double_phi(trait):
    """Bound: DRIVER_TOL = 10 x what the float64 CPU reference at tol = 1e-5 shows against long double on this case
    (4.96e-6, tests/cond_kmat_ref.py)."""
    ans, rec, *_ = run(trait, "family")
    x, ref = long_double(trait, "family")
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    var, cov = np.full(x.size, np.nan), np.full((x.size, len(COND)), np.nan)
    var[x], cov[x] = f(ref["var"]), f(ref["cov"])
    _, _, _, p_ld, _ = CK.driver_expected(rec, trait == "binary", var=var, cov=cov, Phi_CC=f(ref["Phi_CC"]))
    ok = np.isfinite(p_ld)
    assert np.array_equal(ok, np.isfinite(ans["pval.cond"]))
    e = float(np.abs(ans["pval.cond"][ok] / p_ld[ok] - 1).max())
    print(f"{trait}: pval.cond against the long-double Phi^K: {e:.3g} (bound {CK.DRIVER_TOL:.3g}), iters <= {int(ans['n.iter'].max())}")
    assert e <= CK.DRIVER_TOL


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_identity_matrix_is_the_closed_form_for_diagonal_sigma(trait):
    ans, rec, *_ = run(trait, "eye")
    x, ref = long_double(trait, "eye")                       # blocks of one sample: Sigma^-1 is 1 / (tau0 / V_i + tau1)
    _, _, _, var, cov, it, _, _, phi_cc = CK.driver_inputs(rec)
    worst = M.scaled_error(phi_cc, ref["Phi_CC"])
    for j, u in zip(np.flatnonzero(x), ref["units"]):
        worst = max(worst, M.scaled_error(CK.unit_matrix(phi_cc, cov[j], var[j]), u))
    print(f"{trait}: K = identity against the closed form: {worst:.3g} (bound {M.PHI_TOL:.3g}), iters <= {int(it.max())}")
    assert worst <= M.PHI_TOL
