"""GPU: seqFitPCA on the HIP operator (sgx_grm_pca: block subspace iteration on kern_tsblock.h around the operator's
product) against numpy.linalg.eigh of the explicit K.

Bounds, from perturbation theory of a symmetric matrix (no measured tolerance).  With r_c = |K u_c - theta_c u_c| the
residual the solver reports and eps = 64 N 2^-53 lambda_1 for the rounding of the product, of the reported residual and
of eigh itself:
    |theta_c - lambda_c|  <= r_c + eps                       (an eigenvalue lies within the residual of a Ritz value)
    sin angle(u_c, v_c)   <= (r_c + eps) / gap_c             (Davis-Kahan; gap_c: from lambda_c to the rest of the spectrum)
The worst ratios found are printed under -s; those of the first MI355X run are in DESIGN.md 8o."""
import warnings

import numpy as np
import pytest

import grm_ref as R
import pca_ref as P

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def _fit(src, **kw):
    from saigegds_amd import seqFitPCA
    args = dict(n_extra=P.N_EXTRA, tol=P.TOL, max_iter=P.MAX_ITER, verbose=False, **P.FILTER)
    args.update(kw)
    return seqFitPCA(src, **args)


def _operator(codes):
    from saigegds_amd._lib import GrmOperator
    return GrmOperator(R.pack(codes), codes.shape[1])


_cache = {}


def driver_case(c):
    """(codes, result with loadings, op.dense(), eigh of it descending) of a driver case, computed once."""
    if c not in _cache:
        n, m, p = c
        codes = P.structured_codes(n, m, p)
        res = _fit(P.source(codes), n_pc=p - 1, snp_loading=True)
        assert res["snp.id"].size == m
        with _operator(codes) as op:
            K = op.dense()
        lam, V = np.linalg.eigh(K)
        _cache[c] = (codes, res, K, lam[::-1].copy(), V[:, ::-1].copy())
    return _cache[c]


@pytest.mark.parametrize("c", P.DRIVER_CASES, ids=P.case_id)
def test_eigenpairs_within_the_residual_bounds(c):
    n, m, p = c
    n_pc = p - 1
    codes, res, K, lam, V = driver_case(c)
    assert res["converged"].all(), (res["resid"], res["eigenval"], res["n.iter"])
    _, lam_ld = P.dense_K(n, m, p)                                     # gaps from the long-double K
    eps = 64 * n * U * lam[0]
    worst_val = worst_sin = 0.0
    for k in range(n_pc):
        r = res["resid"][k]
        assert r <= P.TOL * res["eigenval"][0]
        dv = abs(res["eigenval"][k] - lam[k])
        gap = min(abs(lam_ld[k] - lam_ld[j]) for j in range(n) if j != k)
        s = P.sine(res["eigenvect"][:, k], V[:, k])
        worst_val, worst_sin = max(worst_val, dv / (r + eps)), max(worst_sin, s / ((r + eps) / gap))
        assert dv <= r + eps, (k, dv, r, eps)
        assert s <= (r + eps) / gap, (k, s, r, eps, gap)
    print(f"\n{P.case_id(c)}: rounds {res['n.iter']}, worst |dtheta| / bound = {worst_val:.3g}, "
          f"worst sine / bound = {worst_sin:.3g}, resid / lambda_1 = {res['resid'] / lam[0]}")


@pytest.mark.parametrize("c", P.DRIVER_CASES, ids=P.case_id)
def test_vectors_orthonormal_signs_and_varprop(c):
    n, m, p = c
    codes, res, K, lam, V = driver_case(c)
    E = res["eigenvect"].astype(np.longdouble)
    L = (p - 1) + P.N_EXTRA
    dev = np.abs(E.T @ E - np.eye(p - 1)).max()
    print(f"\n{P.case_id(c)}: max |E'E - I| = {float(dev):.3g} (bound {8 * L * U:.3g})")
    assert dev <= 8 * L * U
    for k in range(p - 1):
        v = res["eigenvect"][:, k]
        assert v[np.argmax(np.abs(v))] > 0
    assert res["TraceXTX"] == pytest.approx(np.trace(K), rel=1e-12)
    np.testing.assert_allclose(res["varprop"], res["eigenval"] / res["TraceXTX"], rtol=1e-15)


@pytest.mark.parametrize("c", P.DRIVER_CASES, ids=P.case_id)
def test_resid_loadings_and_projection(c):
    n, m, p = c
    n_pc = p - 1
    codes, res, K, lam, V = driver_case(c)
    E = np.ascontiguousarray(res["eigenvect"].T)
    with _operator(codes) as op:
        KE = op.crossprod_many(E)
        dots = op.marker_dots(E)
        af, inv = op.marker_table()
    # the residual, recomputed from the product.  The product's own bound (test_gpu_grm_edges.py): 4 E_ORC units of
    # 2^-53 of its amplification amp_i max|u|, amp_i = (1/M) sum_v g^_vi sum_j g^_vj with g^ = (code + 2 af) inv; the
    # solver's residual went through the same product and two rotations, so twice that, over N entries in the norm,
    # plus the rounding of theta u and of the subtraction
    gh = np.where(codes != 3, (codes.astype(np.float64) + 2 * af[:, None]) * inv[:, None], 0.0)
    amp = float(((gh * gh.sum(axis=1)[:, None]).sum(axis=0) / m).max())
    for k in range(n_pc):
        r = np.linalg.norm(KE[k] - res["eigenval"][k] * E[k])
        slack = np.sqrt(n) * np.abs(E[k]).max() * U * (2 * 4 * R.E_ORC * amp + 4 * lam[0])
        print(f"\n{P.case_id(c)} PC{k + 1}: resid {res['resid'][k]:.6g}, recomputed {r:.6g}, slack {slack:.3g}")
        assert abs(r - res["resid"][k]) <= slack, (k, r, res["resid"][k], slack)
    np.testing.assert_array_equal(res["avgfreq"], af)
    np.testing.assert_array_equal(res["scale"], inv)
    # loadings: dot_v(u) / sqrt(M theta) -- theta is u'Ku, so the rows have unit norm up to rounding
    np.testing.assert_allclose(res["snploading"], dots / np.sqrt(m * res["eigenval"])[:, None], rtol=1e-12, atol=1e-15)
    norms = np.linalg.norm(res["snploading"], axis=1)
    assert (np.abs(norms ** 2 - 1) <= 64 * m * U).all(), norms
    from saigegds_amd import pca_project
    ids, scores = pca_project(res, P.source(codes), verbose=False)
    assert ids == res["sample.id"]
    # score = (K u) / theta = u + r / theta, evaluated as two sums of M and N terms of the amplification's size
    tol = res["resid"] / res["eigenval"] + 64 * m * U * amp * np.abs(E).max(axis=1) / res["eigenval"]
    assert (np.abs(scores - res["eigenvect"]).max(axis=0) <= tol).all(), np.abs(scores - res["eigenvect"]).max(axis=0)


def test_same_seed_same_bits():
    c = P.DRIVER_CASES[0]
    codes, res, *_ = driver_case(c)
    again = _fit(P.source(codes), n_pc=c[2] - 1, snp_loading=True)
    for k in ("eigenval", "eigenvect", "resid", "snploading", "varprop"):
        np.testing.assert_array_equal(again[k], res[k])
    assert again["n.iter"] == res["n.iter"]
    other = _fit(P.source(codes), n_pc=c[2] - 1, seed=7)
    assert not np.array_equal(other["eigenvect"], res["eigenvect"])     # (the seed does reach the start block)


def test_sample_order_follows_the_caller():
    c = P.DRIVER_CASES[0]
    codes, res, *_ = driver_case(c)
    order = np.random.default_rng(2).permutation(c[0])
    ids = [res["sample.id"][i] for i in order]
    perm = _fit(P.source(codes), n_pc=c[2] - 1, sample_id=ids)
    assert perm["sample.id"] == ids
    np.testing.assert_array_equal(perm["eigenvect"], res["eigenvect"][order])


def test_golden_file_what_the_residuals_guarantee():
    import os
    from saigegds_amd import seqFitPCA
    from saigegds_amd._lib import GrmOperator
    from saigegds_amd.gds import GdsFile
    fn = os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.gds")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (it need not converge: no structure is planted)
        res = seqFitPCA(fn, n_pc=2, max_iter=30, verbose=False)
    f = GdsFile(fn)
    packed, n, _ = f.dosage_alt_packed()
    ids = np.asarray(f.read("variant.id"))
    rows = np.flatnonzero(np.isin(ids, res["snp.id"]))
    assert rows.size == res["snp.id"].size
    with GrmOperator(np.ascontiguousarray(np.asarray(packed)[rows]), n) as op:
        K = op.dense()
    lam = np.linalg.eigvalsh(K)[::-1]
    eps = 64 * n * U * lam[0]
    assert np.isfinite(res["eigenvect"]).all()
    for k in range(2):
        near = np.abs(lam - res["eigenval"][k]).min()
        print(f"\ngolden PC{k + 1}: theta {res['eigenval'][k]:.9g}, resid {res['resid'][k]:.3g}, nearest eigenvalue at {near:.3g}")
        assert near <= res["resid"][k] + eps
        r = np.linalg.norm(K @ res["eigenvect"][:, k] - res["eigenval"][k] * res["eigenvect"][:, k])
        assert abs(r - res["resid"][k]) <= 64 * n * U * lam[0] * 4
    assert res["eigenval"][0] <= lam[0] + eps                          # a Ritz value never exceeds lambda_1


def test_rank_breakdown_and_the_handle_after_it():
    from saigegds_amd import seqFitPCA
    from saigegds_amd._lib import GrmOperator, SgxRankError
    rng = np.random.default_rng(2)
    five = rng.binomial(2, 0.3, size=(5, 300)).astype(np.uint8)
    codes = np.tile(five, (40, 1))
    with pytest.raises(ValueError, match="span fewer directions than n_pc \\+ n_extra = 12"):
        seqFitPCA(P.source(codes), n_pc=8, n_extra=4, verbose=False, maf=0.0, missing_rate=1.0)
    b = rng.standard_normal(300)
    with GrmOperator(R.pack(codes), 300) as op:
        before = op.crossprod(b)
        with pytest.raises(SgxRankError):
            op.pca(8, rng.standard_normal((12, 300)))
        np.testing.assert_array_equal(op.crossprod(b), before)         # the handle still answers
        ok = op.pca(3, rng.standard_normal((5, 300)), max_iter=50)     # and decomposes what the markers do span
        assert ok["n_converged"] == 3


def test_one_round_is_reported_not_converged():
    c = P.DRIVER_CASES[0]
    codes = P.structured_codes(*c)
    with pytest.warns(UserWarning, match="did not reach tol"):
        res = _fit(P.source(codes), n_pc=c[2] - 1, max_iter=1, tol=1e-14, snp_loading=True)
    assert not res["converged"].any() and res["n.iter"] == 1
    for k in ("eigenval", "eigenvect", "resid", "snploading", "varprop"):
        assert np.isfinite(res[k]).all(), k


def test_two_samples_one_component():
    rng = np.random.default_rng(9)
    codes = rng.binomial(2, 0.4, size=(50, 2)).astype(np.uint8)
    codes[0] = (0, 2)                                                  # (at least one marker that tells the two apart)
    res = _fit(P.source(codes), n_pc=1, maf=0.0, missing_rate=1.0)
    with _operator(codes) as op:
        K = op.dense()
    lam, V = np.linalg.eigh(K)
    assert res["eigenvect"].shape == (2, 1) and res["converged"].all()
    assert abs(res["eigenval"][0] - lam[-1]) <= res["resid"][0] + 64 * 2 * U * lam[-1]
    assert res["eigenvect"][np.argmax(np.abs(res["eigenvect"][:, 0])), 0] > 0


def test_argument_checks_launch_nothing():
    from saigegds_amd._lib import GrmOperator, SgxError, load
    codes = P.structured_codes(*P.DRIVER_CASES[0])
    n, m = codes.shape[1], codes.shape[0]
    with GrmOperator(R.pack(codes), n) as op:
        Q0 = np.random.default_rng(1).standard_normal((6, n))
        for kw in (dict(n_pc=0), dict(n_pc=7), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-1.0),
                   dict(max_iter=0)):
            args = dict(n_pc=2, max_iter=5, tol=1e-6)
            args.update(kw)
            with pytest.raises(SgxError) as e:
                op.pca(args["n_pc"], Q0, max_iter=args["max_iter"], tol=args["tol"])
            assert e.value.code == -1, kw
        L = load()
        ev, rs, vec = np.zeros(2), np.zeros(2), np.full((2, n), 5.0)
        big = np.zeros((65, n))
        assert L.sgx_grm_pca(op._h, 2, 65, big.ctypes.data, n, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data, n,
                             None, 0, None) == -1
        assert L.sgx_grm_pca(op._h, 2, 6, Q0.ctypes.data, n - 1, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data,
                             n, None, 0, None) == -1
        assert L.sgx_grm_pca(op._h, 2, 6, Q0.ctypes.data, n, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data,
                             n - 1, None, 0, None) == -1
        assert L.sgx_grm_pca(op._h, 2, 6, Q0.ctypes.data, n, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data,
                             n, vec.ctypes.data, m - 1, None) == -1
        assert L.sgx_grm_pca(op._h, 2, 6, None, n, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data, n, None, 0,
                             None) == -1
        assert (vec == 5.0).all()
    small = P.structured_codes(10, 8, 2)
    with GrmOperator(R.pack(small), 10) as op:                         # n_block > N
        Q = np.random.default_rng(1).standard_normal((11, 10))
        ev, rs, vec = np.zeros(2), np.zeros(2), np.zeros((2, 10))
        assert L.sgx_grm_pca(op._h, 2, 11, Q.ctypes.data, 10, 5, 1e-6, ev.ctypes.data, rs.ctypes.data, vec.ctypes.data, 10,
                             None, 0, None) == -1
