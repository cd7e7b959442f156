"""The record of the explicit-GRM solve (saigegds_amd/kmat.py) and the one result tuple of the conditional scan's routes,
without a GPU: the stand-in scanners of tests/cond_kmat_ref.py and tests/kmat_ds_ref.py."""
import numpy as np
import pytest


def test_operator_is_the_scanners_where_it_has_one_else_the_devices(monkeypatch):
    from saigegds_amd import _lib
    from saigegds_amd.kmat import KmatSolve
    k = KmatSolve("mat", np.ones(3), np.array([1.0, 0.5]), 7, 1e-3)

    class WithOperator:
        def grm_operator(self, mat):
            return "the scanner's", mat
    assert k.operator(WithOperator()) == ("the scanner's", "mat")
    monkeypatch.setattr(_lib, "ExplicitGrmOperator", lambda mat: ("the device's", mat))
    assert k.operator(object()) == ("the device's", "mat")
    w, tau, maxiter, tol = k.args
    assert w is k.w and tau is k.tau and (maxiter, tol) == (7, 1e-3)
    with pytest.raises(AttributeError):
        k.tol = 1e-9                                        # frozen


@pytest.mark.parametrize("kind", ["hard", "dosage"])
def test_cond_routes_give_n_iter_exactly_with_grm_mat(kind, monkeypatch):
    from cond_kmat_ref import ref_cond_kmat_scanner_factory
    from kmat_ds_ref import kmat_ds_scanner_factory
    from saigegds_amd import cond, seqAssocGLMM_SPA_cond
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    from test_cond import driver_case
    src, mod = driver_case("binary")
    sid, packed = src.sample_id(), src.packed[:40]
    if kind == "hard":
        small, fac = GenotypeSource(sid, packed=packed), ref_cond_kmat_scanner_factory()
    else:
        codes = unpack_dosage_2bit(packed, 1000)
        small, fac = GenotypeSource(sid, dosage=np.where(codes == 3, np.nan, codes * 0.5)), kmat_ds_scanner_factory()
    seen = []
    for name in ("_scan_hard", "_scan_kmat", "_scan_dosage"):
        def spy(*a, _name=name, _real=getattr(cond, name)):
            seen.append((_name, _real(*a)))
            return seen[-1][1]
        monkeypatch.setattr(cond, name, spy)
    for grm, route in ((None, "_scan_hard"), ((sid, np.eye(1000)), "_scan_kmat")):
        ans = seqAssocGLMM_SPA_cond(small, mod, [30], mac=2, verbose=False, scanner_factory=fac, grm_mat=grm)
        name, r = seen.pop()
        assert not seen and name == (route if kind == "hard" else "_scan_dosage")
        assert isinstance(r, cond.CondScan) and r._fields == ("res", "out_c", "S_C", "Phi_CC", "n_iter")
        assert (r.n_iter is None) == (grm is None) == ("n.iter" not in ans)
        assert r.res.shape == (40, 8 + 3 + 1) and r.Phi_CC.shape == (1, 1)
        if grm is not None:
            assert np.array_equal(ans["n.iter"], r.n_iter[r.res[:, 8] != 0]) and r.n_iter.max() > 0
