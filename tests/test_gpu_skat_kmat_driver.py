"""``seqAssocGLMM_spaSKAT(grm_mat=)`` on the device, on the golden file with a model fitted by
``seqFitNullGLMM_SPA(grm_mat=)``.

The driver's steps are taken from the driver itself (``_prepare``, ``_run``: its ``SkatStep``; ``dosage_tables``,
``_unit_tests``) and fed

* ``Scanner.skat_2bit``: the route of the call without ``grm_mat``, whose table must come out bit for bit;
* the long-double Phi^K of tests/skat_kmat_ref.py on the matrix, V and tau the driver must pass: the p-values of the
  call with ``grm_mat`` (solved to r'r <= 1e-12) against ``_unit_tests`` on that reference.

P_RTOL, the bound on a p-value: Phi^K is within PHI_TOL = 5.55e-7 of the reference, scaled by sqrt(Phi_ee Phi_ff), so
the eigenvalues of diag(w) Phi diag(w) move by at most PHI_TOL times its trace, at most m PHI_TOL of their mean
(m <= 130 here); a tail probability p >= 1e-8 of a chi-square mixture moves by at most q f(q) / p < 40 times the
relative change of its scale: 130 * 5.55e-7 * 40 = 2.9e-3.  Measured on an MI355X (the test prints them): 8.3e-11 for
the driver against the reference, 2.2e-15 for CSR against dense storage (MEASURED_P, MEASURED_STORAGE).
"""
import functools
import os

import numpy as np
import pytest

import skat_kmat_ref as M
from saigegds_amd import seqAssocGLMM_spaSKAT, seqFitNullGLMM_SPA, seqFitSparseGRM
from test_fit_grm_mat import GDS, TRAITS, pheno

pytestmark = pytest.mark.gpu
UNITS = [np.arange(1, 41), np.arange(41, 58), np.zeros(0, dtype=np.int64), np.arange(100, 230)]
KW = dict(verbose=False, wbeta=[1, 25])
P_RTOL = 130 * M.PHI_TOL * 40       # measured: MEASURED_P (driver against the reference), MEASURED_STORAGE (CSR against dense)
MEASURED_P, MEASURED_STORAGE = 8.3e-11, 2.2e-15     # a record of one run, not used by the assertions


@functools.lru_cache(maxsize=None)
def fitted():
    sp = seqFitSparseGRM(GDS, rel_cutoff=0.125, verbose=False)
    return sp, seqFitNullGLMM_SPA(TRAITS["binary"][0], pheno(), GDS, trait_type="binary", verbose=False, grm_mat=sp)


def dense_of(sp):
    K = np.zeros((sp.n, sp.n))
    K[sp.i, sp.j] = sp.x
    K[sp.j, sp.i] = sp.x
    return K


def same(a, b, skip=(), q_rtol=0.0):
    """Equal tables but for the columns ``skip``.  q_rtol: Q = sum w^2 S^2 of a call whose score statistics come from
    sgx_skat_kmat_2bit, which agree with sgx_skat_2bit's to 1e-10 relative (another summation order; header of
    tests/test_gpu_skat_kmat.py), so Q to 2e-10 and second-order terms: 3e-10."""
    assert [k for k in a if k not in skip] == [k for k in b if k not in skip]
    for k in a:
        if k not in skip:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape, k
            if k == "Q" and q_rtol:
                assert np.allclose(x, y, rtol=q_rtol, atol=0, equal_nan=True), k
            else:
                assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y), k


def assembled(mod, sp):
    """The driver's steps from their parts -> (Q, pval) of the variance-ratio route (skat_2bit), pval of _unit_tests
    on skat_2bit's scores and the long-double Phi^K."""
    from saigegds_amd.aggregate import _prepare, _run, dosage_tables
    from saigegds_amd.skat import _unit_tests
    pr = _prepare(GDS, mod, UNITS, KW["wbeta"], 0.05, float("nan"), False, "SAIGE SKAT analysis:")
    try:
        _run(pr, skat=True)                        # the driver's own device step: one batch, skat_2bit
    finally:
        pr.sc.close()
    [st] = pr.skat
    kept, up, var_idx, score, cov = st.kept, st.unit_ptr, st.var_idx, st.score, st.cov
    lut = dosage_tables(st.flip, st.mean)
    packed = pr.inp.packed_rows_at(np.unique(np.concatenate(UNITS)) - 1)
    S_of = lambda u: score[up[u]:up[u + 1]]      # noqa: E731
    Q0, P0 = _unit_tests(pr, kept, S_of, cov.__getitem__)
    ids = pr.inp.sample_id()
    pos = {s: k for k, s in enumerate(sp.sample_id)}
    ix = np.array([pos[s] for s in ids])
    c = dict(sm=pr.sm, packed=packed, var_idx=var_idx, lut=lut, unit_ptr=up, K=dense_of(sp)[np.ix_(ix, ix)], blocks=None,
             w=np.asarray(mod.V, dtype=np.float64)[pr.inp.ii], tau=np.asarray(mod.tau, dtype=np.float64))
    _, phi_ref, _ = M.phi_units(c, "ld")
    _, P1 = _unit_tests(pr, kept, S_of, lambda u: np.asarray(phi_ref[u], dtype=np.float64))
    return Q0[:, 0], P0[:, 0], P1[:, 0]


def test_driver_on_the_fitted_model(tmp_path):
    sp, mod = fitted()
    base = seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW)
    same(base, seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW, grm_mat=None))
    Q0, P0, P_ref = assembled(mod, sp)
    # grm_mat=None is the route of the parent commit: sgx_skat_2bit, then _unit_tests, bit for bit
    assert np.array_equal(np.asarray(base["Q"]), Q0, equal_nan=True) and np.array_equal(np.asarray(base["pval"]), P0, equal_nan=True)
    ans = seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW, grm_mat=sp)
    same(base, ans, skip=("pval", "n.iter"), q_rtol=3e-10)     # Q, n.var and the summary columns do not move
    it, nv = np.asarray(ans["n.iter"]), np.asarray(ans["n.var"])
    assert np.all(it[nv > 0] >= 1) and np.all(it < 500) and it[2] == 0 and np.isnan(np.asarray(ans["pval"])[2])
    # the p-values against _unit_tests fed the reference's Phi^K
    s = seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW, grm_mat=sp, tol_pcg=1e-12)
    ps, pr_ = np.asarray(s["pval"], dtype=np.float64)[nv > 0], P_ref[nv > 0]
    print("pval, driver against _unit_tests on the reference Phi^K:", float(np.abs(ps / pr_ - 1).max()))
    assert np.all(pr_ >= 1e-8) and np.allclose(ps, pr_, rtol=P_RTOL, atol=0)
    assert not np.allclose(ps, P0[nv > 0], rtol=P_RTOL, atol=0)          # and it is not the variance-ratio route's
    # the same matrix as a saved file: the same table; as a dense pair (shuffled): CSR rows and dense rows are summed
    # in different orders, so the two storages agree as two solves to r'r <= 1e-12 do, within the same bound
    fn = os.path.join(tmp_path, "grm.npz")
    seqFitSparseGRM(GDS, rel_cutoff=0.125, verbose=False, out_fn=fn)
    same(ans, seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW, grm_mat=fn))
    perm = np.random.default_rng(3).permutation(sp.n)
    dense = ([sp.sample_id[k] for k in perm], np.ascontiguousarray(dense_of(sp)[np.ix_(perm, perm)]))
    d = seqAssocGLMM_spaSKAT(GDS, mod, UNITS, **KW, grm_mat=dense, tol_pcg=1e-12)
    same(s, d, skip=("pval", "n.iter"))
    pd = np.asarray(d["pval"], dtype=np.float64)[nv > 0]
    print("pval, CSR against dense storage:", float(np.abs(ps / pd - 1).max()))
    assert np.allclose(pd, ps, rtol=P_RTOL, atol=0)
