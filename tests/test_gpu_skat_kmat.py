"""sgx_skat_kmat_2bit and sgx_kmat_pcg_multi_dev on the device, through the C ABI's ctypes binding.

The references, the case table, the input makers and the recorded tolerance are in tests/skat_kmat_ref.py.

* score: against sgx_skat_2bit's score to the scan's 1e-10 (conftest REL_TOL / Z_FLOOR), NOT bit for bit: the column
  kernel adds its sums per slab of 8192 samples, another order than the Gram kernel of sgx_skat_2bit.
* Phi^K: against the long-double reference at tol = 1e-12, maxiter = 500, scaled by sqrt(Phi_ee Phi_ff), within
  PHI_TOL = 5.55e-7 = 10 x the largest discrepancy of the float64-CG reference against the long-double one over the
  same cases (5.54e-8; measured on the CPU by tests/test_skat_kmat_ref.py).  Every case is compared.
* tie to the fit: Phi^K_jj / AC_j against var1 of the golden variance-ratio tables within FIT_TOL = 1.72e-7.
* tau[1] = 0: tau[0] * Phi^K * var_ratio against sgx_skat_2bit's cov at the scan's own 1e-10; iters all 0 or 1.
"""
import ctypes as C

import numpy as np
import pytest

import skat_kmat_ref as M

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in M.CASES]
_ref = {}


def ld_ref(name):
    if name not in _ref:
        _ref[name] = M.phi_units(M.make_case(name), "ld")
    return _ref[name]


def operator(c):
    from saigegds_amd._lib import ExplicitGrmOperator
    return ExplicitGrmOperator(csr=c["csr"]) if c["storage"] == "csr" else ExplicitGrmOperator(c["K"])


def run(c, unit_ptr=None, var_idx=None, lut=None, tau=None, w=None, tol=M.TOL_SOLVE, calls=1):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    unit_ptr = c["unit_ptr"] if unit_ptr is None else unit_ptr
    var_idx = c["var_idx"] if var_idx is None else var_idx
    lut = c["lut"][var_idx] if lut is None else lut
    out = []
    with Scanner(c["sm"]) as sc, operator(c) as op:
        for _ in range(calls):
            out.append(sc.skat_kmat(op, c["packed"], unit_ptr, var_idx, lut, c["w"] if w is None else w,
                                    c["tau"] if tau is None else tau, maxiter=M.MAXITER, tol=tol))
        s2, c2 = sc.skat_2bit(c["packed"], unit_ptr, var_idx, lut)
    return out if calls > 1 else out[0], (s2, c2)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_1_2_score_and_phi_against_the_long_double_reference(name):
    from conftest import REL_TOL, Z_FLOOR
    c = M.make_case(name)
    S_ref, phi_ref, _ = ld_ref(name)
    (score, covs, iters), (s2, c2) = run(c)
    up = c["unit_ptr"]
    assert len(covs) == len(up) - 1 and score.shape == s2.shape == (up[-1],)
    assert np.all(np.isfinite(score)) and int(iters.max()) < M.MAXITER
    worst = 0.0
    for u, (cov, ref) in enumerate(zip(covs, phi_ref)):
        m = int(up[u + 1] - up[u])
        assert cov.shape == (m, m) and np.array_equal(cov, cov.T), f"{name} unit {u}"
        if m == 0:
            continue
        assert np.all(np.isfinite(cov))
        worst = max(worst, M.scaled_error(cov, ref))
        sd = np.sqrt(np.maximum(np.diag(c2[u]), 0))
        s_u, s2_u = score[up[u]:up[u + 1]], s2[up[u]:up[u + 1]]
        e_s = np.abs(s_u - s2_u) - (REL_TOL * np.abs(s2_u) + Z_FLOOR * sd)
        assert float(e_s.max()) <= 0, f"{name} unit {u}: score off sgx_skat_2bit's by {float(np.abs(s_u - s2_u).max()):.3g}"
        e_r = np.abs(s_u - np.asarray(S_ref[up[u]:up[u + 1]], dtype=np.float64))
        assert np.all(e_r <= REL_TOL * np.abs(s2_u) + Z_FLOOR * sd + 1e-300)
    print(f"{name}: Phi^K off the long-double reference by {worst:.3g} (bound {M.PHI_TOL:.3g}), iters <= {int(iters.max())}")
    assert worst <= M.PHI_TOL, name


@pytest.mark.parametrize("name", ["n61_k3_dense", "n1003_k3_csr", "n4099_k5_csr"])
def test_3_tau1_zero_is_the_weighted_gram(name):
    from conftest import REL_TOL
    c = M.make_case(name)
    sm = c["sm"]
    mu2 = np.ones(sm.n) if sm.quant else np.ascontiguousarray(sm.mu2)
    t0 = float(c["tau"][0])
    (score, covs, iters), (s2, c2) = run(c, tau=[t0, 0.0], w=mu2)
    assert set(np.unique(iters).tolist()) <= {0, 1}
    for cov, ref in zip(covs, c2):
        if cov.size == 0:
            continue
        sd = np.sqrt(np.maximum(np.diag(ref), 0))
        d = np.abs(t0 * cov * sm.var_ratio - ref)
        assert np.all(d <= REL_TOL * sd[:, None] * sd[None, :]), f"{name}: {float(d.max()):.3g}"


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_4_tie_to_the_fit(trait):
    """Phi^K_jj / AC_j of the variance-ratio markers is the table's var1: the same solve at the same tol = 1e-5, with
    the dense K = G'G/M of the markers the fit picks.  Bound: FIT_TOL = 10 x the float64 reference's own distance
    from the table (1.72e-8, tests/skat_kmat_ref.py), relative to var1."""
    from test_fit_grm_mat import dense_grm
    c, ac, var1 = M.fit_case(trait, dense_grm()[1])
    (score, covs, iters), _ = run(c, tol=1e-5)
    e = float(np.abs(np.diag(covs[0]) / ac / var1 - 1).max())
    print(f"{trait}: Phi^K_jj / AC_j against var1: {e:.3g} (bound {M.FIT_TOL:.3g}), iters <= {int(iters.max())}")
    assert e <= M.FIT_TOL


def test_5_guarantees():
    c = M.make_case("n1003_k3_csr")
    up, lut = c["unit_ptr"], c["lut"]
    (a, b), _ = run(c, calls=2)
    assert same_bits(a[0], b[0]) and all(same_bits(x, y) for x, y in zip(a[1], b[1])) and np.array_equal(a[2], b[2])
    assert all(np.array_equal(x, x.T) for x in a[1])
    # the last unit (65 entries) alone, and with a unit behind it
    v65 = np.arange(up[2], up[3], dtype=np.int32)
    (s1, c1, i1), _ = run(c, unit_ptr=[0, 65], var_idx=v65)
    assert same_bits(s1, a[0][up[2]:]) and same_bits(c1[0], a[1][2]) and np.array_equal(i1, a[2][up[2]:])
    (s3, c3, i3), _ = run(c, unit_ptr=[0, 65, 65 + 17], var_idx=np.concatenate([v65, np.arange(17, dtype=np.int32)]))
    assert same_bits(s3[:65], s1) and same_bits(c3[0], c1[0]) and np.array_equal(i3[:65], i1)
    # other columns fall into the second 64-chunk: entry 3 becomes the 65th
    perm = np.arange(65)
    perm[[3, 64]] = perm[[64, 3]]
    (sp, cp, ip), _ = run(c, unit_ptr=[0, 65], var_idx=v65[perm])
    inv = np.argsort(perm)
    assert same_bits(sp[inv], s1) and np.array_equal(ip[inv], i1)
    assert same_bits(np.ascontiguousarray(cp[0][np.ix_(inv, inv)]), c1[0])


def test_6_a_non_finite_table_poisons_its_own_row_and_column():
    c = M.make_case("n61_k1_csr")
    up = c["unit_ptr"]
    (s0, c0, _), _ = run(c)
    lut = c["lut"].copy()
    e = int(up[3]) + 5                        # entry 5 of the unit of 17
    lut[e, 3] = np.nan
    (s1, c1, i1), _ = run(c, lut=lut)
    keep = np.arange(up[-1]) != e
    assert np.isnan(s1[e]) and same_bits(s1[keep], s0[keep]) and i1[e] == 0
    for u in range(len(up) - 1):
        if u != 3:
            assert same_bits(c1[u], c0[u])
    k = np.arange(17) != 5
    assert np.all(np.isnan(c1[3][5])) and np.all(np.isnan(c1[3][:, 5]))
    assert same_bits(np.ascontiguousarray(c1[3][np.ix_(k, k)]), np.ascontiguousarray(c0[3][np.ix_(k, k)]))


def test_7_errors_launch_nothing_and_leave_the_handles_usable():
    import torch  # noqa: F401
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner, SgxError, SKAT_MAX_VARIANTS
    c = M.make_case("n61_k1_csr")
    sm, packed, up, vi, lut, w, tau = c["sm"], c["packed"], c["unit_ptr"], c["var_idx"], c["lut"], c["w"], c["tau"]
    with Scanner(sm) as sc, operator(c) as op, ExplicitGrmOperator(np.eye(60)) as op60:
        good = sc.skat_kmat(op, packed, up, vi, lut, w, tau, tol=M.TOL_SOLVE)
        L, h = sc._L, sc._h
        score, cov, it = np.zeros(up[-1]), np.zeros(int((np.diff(up) ** 2).sum())), np.zeros(up[-1], dtype=np.int32)

        def raw(**kw):
            a = dict(h=h, km=op._h, packed=packed.ctypes.data, idx=vi.ctypes.data, up=up.ctypes.data, lut=lut.ctypes.data,
                     w=w.ctypes.data, tau=tau.ctypes.data, score=score.ctypes.data, cov=cov.ctypes.data)
            a.update(kw)
            return L.sgx_skat_kmat_2bit(a["h"], a["km"], a["packed"], packed.shape[1], packed.shape[0], len(up) - 1, a["up"],
                                        a["idx"], a["lut"], a["w"], a["tau"], 500, 1e-12, a["score"], a["cov"], it.ctypes.data)

        for k in ("packed", "idx", "up", "lut", "w", "tau", "score", "cov", "km"):
            assert raw(**{k: None}) == -1, k
        assert raw(km=op60._h) == -1                                   # another sample count
        for bad_w in (0.0, -1.0, np.nan, np.inf):
            w2 = w.copy()
            w2[7] = bad_w
            assert raw(w=w2.ctypes.data) == -1, bad_w
        for bad_tau in ([0.0, 0.5], [-1.0, 0.5], [1.0, -0.1], [np.nan, 0.1]):
            t2 = np.array(bad_tau)
            assert raw(tau=t2.ctypes.data) == -1, bad_tau
        for bad_idx in (-1, packed.shape[0]):
            v2 = vi.copy()
            v2[3] = bad_idx
            assert raw(idx=v2.ctypes.data) == -1, bad_idx
        with pytest.raises(SgxError):
            big = np.zeros(SKAT_MAX_VARIANTS + 1, dtype=np.int32)
            sc.skat_kmat(op, packed, [0, big.size], big, np.tile(lut[0], (big.size, 1)), w, tau)
        assert np.all(score == 0) and np.all(cov == 0)
        again = sc.skat_kmat(op, packed, up, vi, lut, w, tau, tol=M.TOL_SOLVE)
        assert same_bits(again[0], good[0]) and all(same_bits(x, y) for x, y in zip(again[1], good[1]))
        s2, _ = sc.skat_2bit(packed, up, vi, lut)
        assert np.all(np.isfinite(s2))


@pytest.mark.parametrize("name", ["n1003_k3_csr", "n1003_k5_dense"])
@pytest.mark.parametrize("k", [1, 16, 64])
def test_8_the_device_form_of_the_solve_equals_the_host_form(name, k):
    import torch
    c = M.make_case(name)
    n = c["n"]
    B = np.random.default_rng(k).standard_normal((k, n))
    ldb = n + 5
    with operator(c) as op:
        X, it = op.pcg_many(c["w"], c["tau"], B, maxiter=500, tol=1e-9)
        w_d = torch.from_numpy(c["w"]).cuda()
        B_d = torch.zeros((k, ldb), dtype=torch.float64, device="cuda")
        B_d[:, :n] = torch.from_numpy(B).cuda()
        X_d = torch.zeros_like(B_d)
        torch.cuda.synchronize()
        it_d = op.pcg_many_dev(w_d.data_ptr(), c["tau"], B_d.data_ptr(), ldb, k, X_d.data_ptr(), maxiter=500, tol=1e-9)
        Xh = X_d.cpu().numpy()
    assert np.array_equal(it_d, it) and same_bits(np.ascontiguousarray(Xh[:, :n]), X) and np.all(Xh[:, n:] == 0)


def test_9_rows_uploaded_in_chunks():
    """sgx_skat_kmat_2bit sends its rows up as sgx_skat_2bit does, in chunks of pipe_mb MiB at the device stride
    4 ceil(N / 16): 17 504 bytes at N = 70 001, so pipe_mb = 1 is 59 rows a chunk.  60 rows (a chunk and one row) and
    125 (two chunks and a tail of 7, not a multiple of 16), two units whose entries point across the chunks, K = 2, on
    a GRM of pairs: the bits of the one-chunk call."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = M.chunk_case(125, 41)
    packed, lut = c["packed"], c["lut"]
    with Scanner(c["sm"]) as sc, operator(c) as op:
        try:
            for rows, cut in ((60, 17), (125, 40)):
                idx = np.random.default_rng(rows).permutation(rows)
                got = {}
                for pipe_mb in (0, 1):
                    sc.set_option("pipe_mb", pipe_mb)
                    got[pipe_mb] = sc.skat_kmat(op, packed[:rows], [0, cut, rows], idx, lut[idx], c["w"], c["tau"],
                                                maxiter=M.MAXITER, tol=M.TOL_SOLVE)
                keep = np.flatnonzero(np.isfinite(got[0][0]))
                assert keep.size >= rows - 2                 # (the monomorphic row has no finite statistics)
                assert got[0][0].tobytes() == got[1][0].tobytes() and np.array_equal(got[0][2], got[1][2]), rows
                for a, b in zip(got[0][1], got[1][1]):
                    assert a.tobytes() == b.tobytes(), rows
        finally:
            sc.set_option("pipe_mb", 0)
