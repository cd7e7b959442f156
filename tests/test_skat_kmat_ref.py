"""The references of SKAT on an explicit GRM against each other (tests/skat_kmat_ref.py, no GPU): the float64 CG form
against the long-double direct solve over the case table of tests/test_gpu_skat_kmat.py (this is where the recorded
tolerance comes from), the tau[1] = 0 closed form, symmetry, positive semi-definiteness; and the refusals of
``seqAssocGLMM_spaSKAT(grm_mat=)`` with a scanner stand-in."""
import dataclasses

import numpy as np
import pytest

import skat_kmat_ref as M
from test_skat import driver_case, ref_scanner_factory

_memo = {}


def both(name):
    if name not in _memo:
        c = M.make_case(name)
        _memo[name] = (M.phi_units(c, "f64"), M.phi_units(c, "ld"))
    return _memo[name]


def test_f64_against_long_double():
    worst = 0.0
    for name in [c[0] for c in M.CASES]:
        (S64, P64, it), (Sl, Pl, _) = both(name)
        assert int(it.max()) < M.MAXITER, f"{name}: the float64 CG did not converge"
        e = max(M.scaled_error(a, b) for a, b in zip(P64, Pl))
        print(f"{name}: f64 against long double {e:.3g}, iters <= {int(it.max())}")
        worst = max(worst, e)
        assert np.allclose(S64, np.asarray(Sl, dtype=np.float64), rtol=1e-10, atol=1e-10)
    print(f"largest discrepancy {worst:.3g}; recorded {M.REF_DISCREPANCY:.3g}, device bound {M.PHI_TOL:.3g}")
    assert worst <= M.REF_DISCREPANCY


@pytest.mark.parametrize("name", ["n61_k3_dense", "n1003_k3_csr"])
def test_symmetric_and_positive_semi_definite(name):
    (_, P64, _), (_, Pl, _) = both(name)
    for p64, pl in zip(P64, Pl):
        assert np.array_equal(p64, p64.T) and np.array_equal(pl, pl.T)
        if pl.size:
            ev = np.linalg.eigvalsh(np.asarray(pl, dtype=np.float64))
            assert ev.min() >= -1e-12 * max(float(np.diag(pl).max()), 1e-300)


@pytest.mark.parametrize("name", ["n61_k1_csr", "n1003_k1_dense_q"])
def test_tau1_zero_closed_form(name):
    c = M.make_case(name)
    t0 = float(c["tau"][0])
    for form in ("f64", "ld"):
        dt = np.float64 if form == "f64" else np.longdouble
        S, P, it = M.phi_units(c, form, tau=[t0, 0.0])
        A, _ = M.adj_columns(c["sm"], c["packed"], c["var_idx"], c["lut"], dt)
        up = c["unit_ptr"]
        for u, p in enumerate(P):
            a = A[up[u]:up[u + 1]]
            closed = (a * np.asarray(c["w"], dtype=dt)) @ a.T / dt(t0)
            assert M.scaled_error(p, closed) <= 1e-12
        if it is not None:
            assert set(np.unique(it).tolist()) <= {0, 1}


def test_driver_refusals():
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    src, mod, units, codes = driver_case("binary")
    ids = src.sample_id()
    K = (ids, np.eye(len(ids)))
    fac = ref_scanner_factory()
    kw = dict(verbose=False, scanner_factory=fac)
    with pytest.raises(NotImplementedError):
        seqAssocGLMM_spaSKAT(src, mod, units, dsnode="annotation/format/DS", grm_mat=K, **kw)
    frac = GenotypeSource(ids, dosage=np.where(codes == 3, np.nan, codes * 0.5))
    with pytest.raises(NotImplementedError, match="grm_mat"):
        seqAssocGLMM_spaSKAT(frac, mod, units[:2], grm_mat=K, **kw)
    loco = dataclasses.replace(mod, loco={"1": {"tau": np.asarray(mod.tau)}})
    with pytest.raises((ValueError, NotImplementedError)):
        seqAssocGLMM_spaSKAT(src, loco, units, grm_mat=K, **kw)
    with pytest.raises(ValueError, match="not in 'grm_mat'"):
        seqAssocGLMM_spaSKAT(src, mod, units, grm_mat=(ids[:-3], np.eye(len(ids) - 3)), **kw)
    with pytest.raises(ValueError, match="parallel"):
        seqAssocGLMM_spaSKAT(src, mod, units, grm_mat=K, parallel=2, **kw)
    assert fac.calls == 0                       # nothing reached the scanner


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_tie_to_the_fit_on_the_cpu(trait):
    """Where FIT_DISCREPANCY comes from: the float64 reference at tol = 1e-5 against var1 of the golden table."""
    from test_fit_grm_mat import dense_grm
    c, ac, var1 = M.fit_case(trait, dense_grm()[1])
    _, P, it = M.phi_units(c, "f64", tol=1e-5)
    e = float(np.abs(np.diag(P[0]) / ac / var1 - 1).max())
    print(f"{trait}: Phi^K_jj / AC_j against var1: {e:.3g} (recorded {M.FIT_DISCREPANCY:.3g}), iters <= {int(it.max())}")
    assert e <= M.FIT_DISCREPANCY
