"""The references of the conditional scan on an explicit GRM against each other (tests/cond_kmat_ref.py, no GPU): the
float64 CG form against the long-double direct solve over the case table of tests/test_gpu_cond_kmat.py, the tau[1] = 0
closed form, and the driver ``seqAssocGLMM_SPA_cond(grm_mat=)`` with a scanner stand-in: its columns, its algebra, what
it refuses, and the distance of its float64 form from long double that bounds the device's driver."""
import dataclasses

import numpy as np
import pytest

import cond_kmat_ref as CK
import skat_kmat_ref as M
from test_cond import driver_case

COND = [30, 77]


def test_f64_against_long_double():
    worst = 0.0
    for name in [c[0] for c in CK.CASES]:
        a, b = CK.case_ref(name, "f64"), CK.case_ref(name, "ld")
        assert int(a["iters"].max()) < M.MAXITER, f"{name}: the float64 CG did not converge"
        e = max([M.scaled_error(a["Phi_CC"], b["Phi_CC"])] + [M.scaled_error(x, y) for x, y in zip(a["units"], b["units"])])
        print(f"{name}: f64 against long double {e:.3g}, iters <= {int(a['iters'].max())}")
        worst = max(worst, e)
    print(f"largest discrepancy {worst:.3g}; the project's REF_DISCREPANCY {M.REF_DISCREPANCY:.3g}, device bound {M.PHI_TOL:.3g}")
    assert worst <= M.REF_DISCREPANCY


@pytest.mark.parametrize("name", ["n61_k1_c1_csr", "n1003_k3_c7_csr"])
def test_tau1_zero_closed_form(name):
    c = CK.make_case(name)
    t0, nc = float(c["tau"][0]), c["n_cond"]
    for form in ("f64", "ld"):
        dt = np.float64 if form == "f64" else np.longdouble
        r = CK.phi_rows(c["sm"], c["packed"], c["lut"], nc, c["K"], c["w"], [t0, 0.0], form, c["blocks"])
        A, _ = M.adj_columns(c["sm"], c["packed"], c["var_idx"], c["lut"], dt)
        closed = (A * np.asarray(c["w"], dtype=dt)) @ A.T / dt(t0)
        for j, u in enumerate(r["units"]):
            idx = list(range(nc)) + [nc + j]
            assert M.scaled_error(u, closed[np.ix_(idx, idx)]) <= 1e-12
        if r["iters"] is not None:
            assert set(np.unique(r["iters"]).tolist()) <= {0, 1}


def family(n=1000):
    K, _, blocks = M.family_K(n)
    return K, blocks


def run_driver(trait, form, tol=1e-5, **kw):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    src, mod = driver_case(trait)
    K, blocks = family()
    fac = CK.ref_cond_kmat_scanner_factory(form, blocks)
    ans = seqAssocGLMM_SPA_cond(src, mod, COND, mac=4, verbose=False, scanner_factory=fac, grm_mat=(src.sample_id(), K),
                                tol_pcg=tol, **kw)
    return ans, fac.last


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_driver_with_reference_scanner(trait):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from test_cond import ref_cond_scanner_factory
    src, mod = driver_case(trait)
    plain = seqAssocGLMM_SPA_cond(src, mod, COND, mac=4, verbose=False, scanner_factory=ref_cond_scanner_factory())
    none = seqAssocGLMM_SPA_cond(src, mod, COND, mac=4, verbose=False, scanner_factory=ref_cond_scanner_factory(),
                                 grm_mat=None, tol_pcg=1e-3, maxiter_pcg=7)
    assert list(none.keys()) == list(plain.keys())
    for k in plain:
        assert np.array_equal(np.asarray(none[k]), np.asarray(plain[k]), equal_nan=True) if np.asarray(plain[k]).dtype.kind == "f" \
            else list(none[k]) == list(plain[k]), k
    ans, rec = run_driver(trait, "f64")
    assert list(ans.keys()) == list(plain.keys()) + ["n.iter"]
    ids = list(ans["id"])
    assert ids == list(plain["id"])
    for col in ("beta.cond", "SE.cond", "pval.cond"):
        a = ans[col]
        assert np.isnan(a[ids.index(30)]) and np.isnan(a[ids.index(77)])
        assert np.isfinite(np.delete(a, [ids.index(30), ids.index(77)])).all()
    # the driver's algebra: cond_tests on the scanner's own outputs, SPA scale factors against Phi^K_jj
    x, beta, se, p, it = CK.driver_expected(rec, trait == "binary")
    assert int(x.sum()) == len(ids) and len(rec.sets) == 1
    for col, want in (("beta.cond", beta), ("SE.cond", se), ("pval.cond", p)):
        assert np.array_equal(ans[col], want, equal_nan=True), col
    assert np.array_equal(ans["n.iter"], it) and ans["n.iter"].max() > 0
    # rows that fail the thresholds reach cond_kmat with NaN tables: no solve
    _, _, S, var, _, it_all, _, _, _ = CK.driver_inputs(rec)
    assert (~x).sum() >= 2 and np.all(np.isnan(var[~x])) and np.all(it_all[~x] == 0)
    # var_ratio does not enter Phi^K (it still moves the scan's own columns, and through pval the SPA scale factors)
    _, rec2 = run_driver(trait, "f64", var_ratio=2.0)
    for k in (3, 4, 8):
        assert np.array_equal(CK.driver_inputs(rec2)[k], CK.driver_inputs(rec)[k], equal_nan=True)


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_driver_pval_of_the_f64_reference_against_long_double(trait):
    """Where DRIVER_DISCREPANCY comes from: pval.cond from the float64 CG at tol = 1e-5 against cond_tests fed the
    long-double Phi^K, relative."""
    ans, rec = run_driver(trait, "f64")
    _, rec_ld = run_driver(trait, "ld")
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    _, _, _, var, cov, _, _, _, phi = CK.driver_inputs(rec_ld)
    _, _, _, p_ld, _ = CK.driver_expected(rec, trait == "binary", var=f(var), cov=f(cov), Phi_CC=f(phi))
    ok = np.isfinite(p_ld)
    assert np.array_equal(ok, np.isfinite(ans["pval.cond"]))
    e = float(np.abs(ans["pval.cond"][ok] / p_ld[ok] - 1).max())
    print(f"{trait}: pval.cond of the float64 reference at tol = 1e-5 against long double: {e:.3g} "
          f"(recorded {CK.DRIVER_DISCREPANCY:.3g}), iters <= {int(ans['n.iter'].max())}")
    assert e <= CK.DRIVER_DISCREPANCY


def test_driver_refusals():
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from saigegds_amd.assoc import GenotypeSource
    src, mod = driver_case("binary")
    ids = src.sample_id()
    K = (ids, np.eye(len(ids)))
    fac = CK.ref_cond_kmat_scanner_factory()
    kw = dict(verbose=False, scanner_factory=fac)
    with pytest.raises(NotImplementedError):
        seqAssocGLMM_SPA_cond(src, mod, COND, dsnode="annotation/format/DS", grm_mat=K, **kw)
    ds = GenotypeSource(ids, dosage=np.full((4, 1000), 0.5))
    with pytest.raises(NotImplementedError, match="grm_mat"):
        seqAssocGLMM_SPA_cond(ds, mod, [1], grm_mat=K, **kw)
    loco = dataclasses.replace(mod, loco={"1": {"tau": np.asarray(mod.tau)}})
    with pytest.raises(NotImplementedError, match="leave-one-chromosome-out"):
        seqAssocGLMM_SPA_cond(src, loco, COND, grm_mat=K, **kw)
    with pytest.raises(ValueError, match="not in 'grm_mat'"):
        seqAssocGLMM_SPA_cond(src, mod, COND, grm_mat=(ids[:-3], np.eye(len(ids) - 3)), **kw)
    assert fac.calls == 0                       # nothing reached the scanner


def test_abi_declared_and_bound():
    import os
    import re
    from saigegds_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "saigehip.h")) as f:
        hdr = f.read()
    with open(_lib.__file__) as f:
        lib = f.read()
    for fn in ("sgx_cond_kmat_set", "sgx_cond_kmat_2bit"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr) and '"%s"' % fn in lib
    assert hasattr(_lib.Scanner, "cond_kmat_set") and hasattr(_lib.Scanner, "cond_kmat")
