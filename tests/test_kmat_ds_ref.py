"""SKAT and the conditional scan on an explicit GRM from dosage rows without a GPU (tests/kmat_ds_ref.py):
the float64 CG reference against the long-double direct solve over the case table of tests/test_gpu_kmat_ds.py (where
the device bound comes from), hard calls as dosage rows against the 2-bit reference, the two drivers with the numpy
stand-in blocks, the distance of their float64 form from long double that bounds the device's drivers, the refusals,
and the C ABI's declaration and binding."""
import os
import re

import numpy as np
import pytest

import kmat_ds_ref as KD
import skat_ds_ref as SD
import skat_kmat_ref as M

NAMES = [c[0] for c in KD.CASES]


def test_f64_against_long_double():
    worst = 0.0
    for name in NAMES:
        a, b = KD.case_ref(name, "f64"), KD.case_ref(name, "ld")
        assert int(a["iters"].max()) < M.MAXITER, f"{name}: the float64 CG did not converge"
        pairs = list(zip(a["skat"], b["skat"])) + [(a["Phi_CC"], b["Phi_CC"])] + list(zip(a["units"], b["units"]))
        e = max(KD.finite_error(x, y) for x, y in pairs)
        print(f"{name}: f64 against long double {e:.3g}, iters <= {int(a['iters'].max())}")
        worst = max(worst, e)
        assert np.allclose(a["S"], np.asarray(b["S"], dtype=np.float64), rtol=1e-10, atol=1e-10, equal_nan=True)
        bad = ~np.isfinite(KD.make_case(name)["mean"])
        assert np.array_equal(np.isnan(a["S"]), bad) and np.all(a["iters"][bad] == 0)
    print(f"largest discrepancy {worst:.3g}; recorded {KD.RECORDED_REF:.3g}, the project's REF_DISCREPANCY "
          f"{M.REF_DISCREPANCY:.3g}, device bound {M.PHI_TOL:.3g}")
    assert worst <= KD.RECORDED_REF <= M.REF_DISCREPANCY


def test_the_case_table_reaches_every_edge():
    t = KD.CASES
    assert {c[1] for c in t} == {61, 1003, 4099, 8195} and {c[2] for c in t} == {1, 3, 5, 16}
    assert {np.dtype(c[5]) for c in t} == {np.dtype(np.uint8), np.dtype(np.float64), np.dtype(np.int32)}
    assert {c[6] for c in t} == {True, False} and {c[4] for c in t} == {"csr", "dense"}
    assert {1, 16, 17, 65} <= {m for c in t for m in c[7]} and {1, 7, 16} == {c[8] for c in t}
    assert {1, 63, 64, 65} <= {c[9] for c in t}
    for name in NAMES:
        c = KD.make_case(name)
        assert c["flip"].any() and not c["flip"].all(), name                       # flipped and unflipped entries
        zero = np.array([np.all(np.where(SD.ok_mask(r), r, 0) == 0) and SD.ok_mask(r).any() for r in c["rows"]])
        assert zero.any(), name                                                     # a row of equal values
        gone = np.array([not SD.ok_mask(r).any() for r in c["rows"]])
        assert gone.any() == bool(next(x for x in t if x[0] == name)[6]), name      # a row with every sample missing


@pytest.mark.parametrize("name", ["n61_k1_csr", "n1003_k5_dense"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float64, np.int32])
def test_hard_calls_as_dosage_rows_equal_the_packed_reference(name, dtype):
    c = M.make_case(name)
    rows = KD.as_block_rows(c["codes"], dtype)
    flip, mean = SD.flip_mean(rows)
    c2 = dict(c, rows=rows, flip=flip, mean=mean)
    S, P, it = KD.phi_units(c2, "f64")
    S0, P0, it0 = M.phi_units(c, "f64")
    assert np.array_equal(it, it0)
    assert np.allclose(S, S0, rtol=1e-13, atol=1e-13)
    for p, p0 in zip(P, P0):
        assert M.scaled_error(p, p0) <= 1e-13


# ---- the drivers with the stand-in blocks ---------------------------------------------------------------------------
def family(n=1000):
    K, _, blocks = M.family_K(n)
    return K, blocks


def skat_case():
    from saigegds_amd.assoc import GenotypeSource
    from test_skat_dosage import fractional_case, _model
    ds, sid, _ = fractional_case(n_var=100)
    units = [np.arange(s, s + 12) + 1 for s in range(0, 88, 8)]
    return GenotypeSource(sid, dosage=ds), _model("binary"), units


def run_skat(form, tol=1e-5, **kw):
    from saigegds_amd import seqAssocGLMM_spaSKAT
    src, mod, units = skat_case()
    K, blocks = family()
    fac = KD.kmat_ds_scanner_factory(form, blocks)
    ans = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=fac, grm_mat=(src.sample_id(), K),
                               tol_pcg=tol, **kw)
    return ans, fac.last


def test_skat_driver_on_a_float64_dosage_source():
    from saigegds_amd import aggregate, skat
    one, sc1 = run_skat("f64")
    assert sc1.uploads == 1 and len(sc1.kmat_log) == 1 and "n.iter" in one
    many, scm = run_skat("f64", ds_budget=30 * 8000)
    assert scm.uploads >= 3 and len(scm.kmat_log) == scm.uploads
    assert list(one) == list(many)
    for k in one:                           # (the stand-in's matrix products round by their shapes: not bit for bit)
        assert np.allclose(np.asarray(one[k]), np.asarray(many[k]), rtol=1e-8, atol=0, equal_nan=True), k
    assert np.isfinite(one["pval.b1_25"]).all() and one["n.iter"].max() > 0
    # the driver's algebra: _unit_tests on the stand-in's own Phi^K (SPA scale factors against Phi^K_jj)
    calls = []
    real = skat._unit_tests

    def spy(pr, kept, S_of, phi_of):
        calls.append((pr, kept, [S_of(u) for u in range(len(kept))], [phi_of(u) for u in range(len(kept))]))
        return real(pr, kept, S_of, phi_of)
    skat._unit_tests = spy
    try:
        again, sc = run_skat("f64")
    finally:
        skat._unit_tests = real
    pr, kept, S, Phi = calls[0]
    score, covs, iters = sc.kmat_log[0][1]
    assert len(covs) == len(Phi) and all(np.array_equal(a, b) for a, b in zip(covs, Phi))
    assert np.array_equal(np.concatenate(S), score)
    Q, P = real(pr, kept, S.__getitem__, covs.__getitem__)
    assert np.array_equal(again["Q.b1_25"], Q[:, 1]) and np.array_equal(again["pval.b1_25"], P[:, 1])
    up = np.concatenate([[0], np.cumsum([k.size for k in kept])])
    assert np.array_equal(again["n.iter"], [iters[a:b].max() for a, b in zip(up[:-1], up[1:])])
    assert aggregate.DS_BUDGET == 1 << 30


def run_cond(form, tol=1e-5, **kw):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from test_cond_dosage import fractional_case
    src, mod = fractional_case("binary")
    K, blocks = family()
    fac = KD.kmat_ds_scanner_factory(form, blocks)
    ans = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=2, verbose=False, scanner_factory=fac,
                                grm_mat=(src.sample_id(), K), tol_pcg=tol, **kw)
    return ans, fac.last


def cond_expected(sc, var=None, cov=None, Phi_CC=None, spa_pval=0.05):
    """``cond_tests`` on a recorded run's own outputs (or with var, cov, Phi_CC replaced) -> (kept, pval.cond, n.iter)."""
    from saigegds_amd.cond import cond_tests
    from saigegds_amd.skat import spa_scale
    out_c = sc.scan_log[0][0]
    out8 = np.concatenate([o for o, _ in sc.scan_log[1:]])
    valid = np.concatenate([v for _, v in sc.scan_log[1:]])
    S_C, phi0, _ = next(r for k, r in sc.kmat_log if k == "set")
    S, var0, cov0, it = (np.concatenate([r[i] for k, r in sc.kmat_log if k == "rows"]) for i in range(4))
    var, cov, Phi_CC = (var0 if var is None else var), (cov0 if cov is None else cov), (phi0 if Phi_CC is None else Phi_CC)
    x = valid != 0
    order = np.argsort([30 - 1, 77 - 1])           # the set's block holds its rows in ascending order: here as given
    assert list(order) == [0, 1]
    d = spa_scale(out8[x], S[x], var[x], spa_pval)
    d_C = spa_scale(out_c, S_C, np.diag(Phi_CC), spa_pval)
    _, _, p = cond_tests(S[x], var[x], cov[x], S_C, Phi_CC, d, d_C)
    return x, p, it[x], (var0, cov0, phi0)


def test_cond_driver_on_a_dosage_source(monkeypatch):
    from saigegds_amd import aggregate
    ans, sc = run_cond("f64")
    assert sc.uploads == 2 and "n.iter" in ans and list(ans)[-1] == "n.iter"
    x, p, it, (var, _, _) = cond_expected(sc)
    assert np.array_equal(ans["pval.cond"], p, equal_nan=True) and np.array_equal(ans["n.iter"], it)
    assert ans["n.iter"].max() > 0 and np.isfinite(ans["pval.cond"]).sum() >= 150
    # rows that fail the thresholds reach cond_kmat with a NaN mean: no solve
    it_all = np.concatenate([r[3] for k, r in sc.kmat_log if k == "rows"])
    assert (~x).sum() >= 2 and np.all(np.isnan(var[~x])) and np.all(it_all[~x] == 0)
    monkeypatch.setattr(aggregate, "DS_BUDGET", 60 * 1000 * 8)      # 222 rows in 4 batches
    cut, sc2 = run_cond("f64")
    assert sc2.uploads == 1 + 4
    for k in ans:                           # (the stand-in's matrix products round by their shapes: not bit for bit)
        a, b = np.asarray(ans[k]), np.asarray(cut[k])
        assert np.allclose(a, b, rtol=1e-8, atol=0, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), k


def test_driver_pvals_of_the_f64_reference_against_long_double():
    """Where DRIVER_DISCREPANCY comes from: the two drivers' p-values from the float64 CG at tol = 1e-5 against the same
    algebra fed the long-double Phi^K, relative."""
    from saigegds_amd import skat
    ans, sc = run_cond("f64")
    _, sc_ld = run_cond("ld")
    _, _, _, (var, cov, phi) = cond_expected(sc_ld)
    _, p_ld, _, _ = cond_expected(sc, var=var, cov=cov, Phi_CC=phi)
    ok = np.isfinite(p_ld)
    assert np.array_equal(ok, np.isfinite(ans["pval.cond"]))
    e_c = float(np.abs(ans["pval.cond"][ok] / p_ld[ok] - 1).max())
    a64, _ = run_skat("f64")
    ald, _ = run_skat("ld")                # the same S; Phi^K, and through it the SPA scale factors, in long double
    e_s = max(float(np.abs(a64[c] / ald[c] - 1).max()) for c in ("pval.b1_1", "pval.b1_25"))
    assert np.allclose(a64["Q.b1_25"], ald["Q.b1_25"], rtol=1e-12, atol=0)
    print(f"pval.cond of the float64 reference at tol = 1e-5 against long double: {e_c:.3g}; SKAT pval: {e_s:.3g} "
          f"(recorded {KD.DRIVER_DISCREPANCY:.3g})")
    assert max(e_c, e_s) <= KD.DRIVER_DISCREPANCY
    assert skat.LAMBDA_DROP == 1e-10


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from saigegds_amd import seqAssocGLMM_SPA_cond, seqAssocGLMM_spaSKAT
    from saigegds_amd.cond import _NO_DOSAGE_KMAT
    from cond_ds_ref import NumpyCondDsScanner
    from test_cond_dosage import fractional_case
    src, mod, units = skat_case()
    K = (src.sample_id(), np.eye(1000))

    def closing(Base):
        class Fac(Base):
            closed = 0

            def close(self):
                Fac.closed += 1
                super().close()
        return Fac

    # a scanner whose block lacks skat_kmat / cond_kmat: today's grm_mat messages, the scanner closed, nothing read
    Fac = closing(NumpyCondDsScanner)
    with pytest.raises(NotImplementedError, match=re.escape("SKAT with 'grm_mat' on dosage input is not implemented.")):
        seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=Fac, grm_mat=K)
    assert Fac.closed >= 1 and Fac.last.uploads == 0
    csrc, cmod = fractional_case("binary")
    Fac = closing(NumpyCondDsScanner)
    with pytest.raises(NotImplementedError, match=re.escape(_NO_DOSAGE_KMAT)):
        seqAssocGLMM_SPA_cond(csrc, cmod, [30], verbose=False, scanner_factory=Fac, grm_mat=K)
    assert Fac.closed >= 1 and Fac.last.uploads == 0
    # a scanner without dosage_block
    from test_skat import ref_scanner_factory
    from test_cond import ref_cond_scanner_factory
    with pytest.raises(NotImplementedError, match="grm_mat"):
        seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=closing(ref_scanner_factory()), grm_mat=K)
    with pytest.raises(NotImplementedError, match="grm_mat"):
        seqAssocGLMM_SPA_cond(csrc, cmod, [30], verbose=False, scanner_factory=ref_cond_scanner_factory(), grm_mat=K)
    # LOCO models and more than one GPU stay refused
    import dataclasses
    loco = dataclasses.replace(mod, loco={"1": {"tau": np.asarray(mod.tau)}})
    good = KD.kmat_ds_scanner_factory()
    with pytest.raises((ValueError, NotImplementedError)):
        seqAssocGLMM_spaSKAT(src, loco, units, verbose=False, scanner_factory=good, grm_mat=K)
    with pytest.raises(ValueError, match="parallel"):
        seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=good, grm_mat=K, parallel=2)
    assert good.last is None


def test_abi_declared_and_bound():
    from saigegds_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "saigehip.h")) as f:
        hdr = f.read()
    for fn in ("sgx_ds_block_skat_kmat", "sgx_ds_block_cond_kmat_set", "sgx_ds_block_cond_kmat"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr) and fn in _lib.ABI, fn
    for m in ("skat_kmat", "cond_kmat_set", "cond_kmat"):
        assert hasattr(_lib.DosageBlock, m), m
