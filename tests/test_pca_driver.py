"""CPU: the host logic of seqFitPCA / pca_project (saigegds_amd/pca.py) on the numpy stand-in operator of pca_ref.py:
the result's keys and shapes, the caller's sample order, the sign rule, varprop, the files, the refusals and the
projection of the training samples."""
import warnings

import numpy as np
import pytest

import pca_ref as P

import saigegds_amd
from saigegds_amd import load_pca, pca_project, seqFitPCA

N, M, NPOP = 120, 400, 3
N_PC = 2


@pytest.fixture(scope="module")
def codes():
    return P.structured_codes(N, M, NPOP)


def _fit(codes, **kw):
    args = dict(n_pc=N_PC, n_extra=6, verbose=False, operator_factory=P.NumpyPcaGrm, **P.FILTER)
    args.update(kw)
    return seqFitPCA(P.source(codes), **args)


@pytest.fixture(scope="module")
def fit(codes):
    return _fit(codes, snp_loading=True)


def test_exported_names():
    for name in ("seqFitPCA", "pca_project", "load_pca"):
        assert hasattr(saigegds_amd, name)
    from saigegds_amd._lib import ABI, GrmOperator
    for name in ("sgx_grm_pca", "sgx_grm_marker_dots", "sgx_grm_marker_dots_dev", "sgx_grm_marker_table",
                 "sgx_grm_ts_gram", "sgx_grm_ts_apply"):
        assert name in ABI
    for name in ("pca", "marker_dots", "marker_table", "ts_gram", "ts_apply"):
        assert hasattr(GrmOperator, name)


def test_keys_and_shapes(fit):
    assert set(fit) == {"sample.id", "snp.id", "eigenval", "eigenvect", "varprop", "TraceXTX", "resid", "converged",
                        "n.iter", "snploading", "avgfreq", "scale"}
    assert fit["sample.id"] == [f"s{i}" for i in range(N)]
    assert fit["snp.id"].shape == (M,)
    assert fit["eigenval"].shape == fit["varprop"].shape == fit["resid"].shape == fit["converged"].shape == (N_PC,)
    assert fit["eigenvect"].shape == (N, N_PC)
    assert fit["snploading"].shape == (N_PC, M) and fit["avgfreq"].shape == fit["scale"].shape == (M,)
    assert fit["converged"].dtype == bool and fit["converged"].all()
    assert isinstance(fit["n.iter"], int) and fit["n.iter"] >= 1
    assert (np.diff(fit["eigenval"]) <= 0).all()


def test_without_loadings_no_loading_keys(codes):
    res = _fit(codes)
    assert not {"snploading", "avgfreq", "scale"} & set(res)


def test_eigenpairs_and_varprop(codes, fit):
    K = P.NumpyPcaGrm(P.R.pack(codes), N).K
    lam = np.linalg.eigvalsh(K)[::-1]
    np.testing.assert_allclose(fit["eigenval"], lam[:N_PC], rtol=1e-9)
    assert fit["TraceXTX"] == pytest.approx(np.trace(K), rel=1e-12)
    np.testing.assert_allclose(fit["varprop"], fit["eigenval"] / np.trace(K), rtol=1e-12)
    np.testing.assert_allclose(fit["eigenvect"].T @ fit["eigenvect"], np.eye(N_PC), atol=1e-12)
    r = K @ fit["eigenvect"] - fit["eigenvect"] * fit["eigenval"][None, :]
    np.testing.assert_allclose(np.linalg.norm(r, axis=0), fit["resid"], atol=1e-9 * lam[0])


def test_sign_rule(fit):
    for c in range(N_PC):
        v = fit["eigenvect"][:, c]
        assert v[np.argmax(np.abs(v))] > 0


def test_sample_order_follows_the_caller(codes, fit):
    rng = np.random.default_rng(1)
    order = rng.permutation(N)
    ids = [f"s{i}" for i in order]
    res = _fit(codes, sample_id=ids)
    assert res["sample.id"] == ids
    np.testing.assert_array_equal(res["eigenvect"], fit["eigenvect"][order])
    np.testing.assert_array_equal(res["eigenval"], fit["eigenval"])


@pytest.mark.parametrize("ext", [".rds", ".npz"])
def test_file_round_trip(codes, fit, tmp_path, ext):
    fn = str(tmp_path / ("pca" + ext))
    res = _fit(codes, snp_loading=True, out_fn=fn)
    back = load_pca(fn)
    assert set(back) == set(res)
    assert back["sample.id"] == res["sample.id"] and back["n.iter"] == res["n.iter"]
    assert back["TraceXTX"] == res["TraceXTX"]
    np.testing.assert_array_equal(back["snp.id"], res["snp.id"])
    np.testing.assert_array_equal(back["converged"], res["converged"])
    for k in ("eigenval", "eigenvect", "varprop", "resid", "snploading", "avgfreq", "scale"):
        np.testing.assert_array_equal(back[k], res[k])
    if ext == ".rds":
        from saigegds_amd.rds import read_rds
        r = read_rds(fn)
        assert list(r.names)[:6] == ["sample.id", "snp.id", "eigenval", "eigenvect", "varprop", "resid"]
        assert np.asarray(r["eigenvect"]).shape == (N, N_PC)


def test_bad_out_fn_refused_before_any_work(codes):
    with pytest.raises(ValueError, match="RDS or npz"):
        _fit(codes, out_fn="pca.txt", operator_factory=None)


def test_too_many_components_refused():
    small = P.structured_codes(10, 8, 2)
    with pytest.raises(ValueError, match="n_pc"):
        seqFitPCA(P.source(small), n_pc=9, n_extra=0, verbose=False, operator_factory=P.NumpyPcaGrm, maf=0.0,
                  missing_rate=1.0)


def test_bad_arguments_refused(codes):
    for kw in (dict(n_pc=0), dict(n_extra=-1), dict(tol=float("nan")), dict(tol=-1.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            _fit(codes, **kw)


def test_rank_breakdown_becomes_a_value_error():
    rng = np.random.default_rng(2)
    five = rng.binomial(2, 0.3, size=(5, 60)).astype(np.uint8)
    codes = np.tile(five, (40, 1))
    with pytest.raises(ValueError, match="span fewer directions than n_pc \\+ n_extra = 12"):
        seqFitPCA(P.source(codes), n_pc=8, n_extra=4, verbose=False, operator_factory=P.NumpyPcaGrm, maf=0.0,
                  missing_rate=1.0)


def test_not_converged_warns(codes):
    with pytest.warns(UserWarning, match="did not reach tol"):
        res = _fit(codes, max_iter=1, tol=1e-14)
    assert not res["converged"].any() and res["n.iter"] == 1
    assert np.isfinite(res["eigenvect"]).all() and np.isfinite(res["eigenval"]).all()


def test_converged_does_not_warn(codes):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _fit(codes)


def test_project_needs_loadings(codes):
    with pytest.raises(ValueError, match="snp_loading=True"):
        pca_project(_fit(codes), P.source(codes), verbose=False)


def test_project_training_samples_reproduces_eigenvect(codes, fit):
    ids, scores = pca_project(fit, P.source(codes), verbose=False)
    assert ids == fit["sample.id"] and scores.shape == (N, N_PC)
    # score = K u / theta = u + r / theta: within resid / theta of eigenvect, plus rounding
    tol = fit["resid"] / fit["eigenval"] + 1e-12
    assert (np.abs(scores - fit["eigenvect"]).max(axis=0) <= tol).all()
    sub = [f"s{i}" for i in (7, 3, 99)]
    ids2, s2 = pca_project(fit, P.source(codes), sample_id=sub, verbose=False)
    assert ids2 == sub
    np.testing.assert_allclose(s2, scores[[7, 3, 99]], rtol=0, atol=1e-13)


def test_project_from_a_gds_file():
    """The file branch of pca_project's row reader: runs of consecutive rows of the golden file, all samples and a
    subset in another order.  score = (K u) / theta = u + r / theta, converged or not."""
    import os
    fn = os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.gds")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (3 rounds without planted structure)
        res = seqFitPCA(fn, n_pc=2, n_extra=4, max_iter=3, max_num_snp=600, snp_loading=True, verbose=False,
                        operator_factory=P.NumpyPcaGrm)
    m = res["snp.id"].size
    assert 0 < m <= 600 and (np.diff(np.sort(res["snp.id"])) > 1).any()   # (a random subset: several runs of rows)
    ids, scores = pca_project(res, fn, verbose=False)
    assert ids == res["sample.id"] and scores.shape == (len(ids), 2)
    tol = res["resid"] / res["eigenval"] + 1e-12
    assert (np.abs(scores - res["eigenvect"]).max(axis=0) <= tol).all()
    assert np.abs(scores - res["eigenvect"]).max() > 0                 # (not converged: the residual is really there)
    sub = [ids[k] for k in (900, 5, 431, 17)]
    ids2, s2 = pca_project(res, fn, sample_id=sub, verbose=False)
    assert ids2 == sub
    np.testing.assert_allclose(s2, scores[[900, 5, 431, 17]], rtol=0, atol=1e-13)


def test_project_pass_is_sized_by_bytes(codes, fit, monkeypatch):
    import saigegds_amd.pca as pca_mod
    _, scores = pca_project(fit, P.source(codes), verbose=False)
    monkeypatch.setattr(pca_mod, "_PROJECT_BYTES", 8 * N * 7)          # 7 marker rows a pass
    _, small = pca_project(fit, P.source(codes), verbose=False)
    np.testing.assert_allclose(small, scores, rtol=0, atol=1e-13)


def test_rank_error_is_matched_by_type(codes):
    from saigegds_amd._lib import PcaRankError, SgxRankError
    assert issubclass(SgxRankError, PcaRankError) and P.PcaRankError is PcaRankError

    class Other(P.NumpyPcaGrm):
        def pca(self, *a, **k):
            class SgxRankError(ValueError):                            # the name alone does not make it one
                pass
            raise SgxRankError("unrelated")

    with pytest.raises(ValueError, match="unrelated"):
        _fit(codes, operator_factory=Other)


def test_project_unknown_marker_refused(codes, fit):
    bad = dict(fit)
    bad["snp.id"] = fit["snp.id"] + 10 ** 6
    with pytest.raises(ValueError, match="snp.id"):
        pca_project(bad, P.source(codes), verbose=False)
