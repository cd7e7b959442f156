"""``sgx_skato_spectra`` (kern_eig.h) and ``seqAssocGLMM_spaSKATO`` on the device: the batched Jacobi
kernel against 40-digit eigenvalues and against numpy at the edges of its size classes and storage, structured
matrices, independence of a problem from its call, the errors, and the driver against its own numpy route."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
RHO = (0, 0.01, 0.04, 0.09, 0.25, 0.5, 1)
EPS = float(np.finfo(np.float64).eps)
# seqAssocGLMM_spaSKATO with the device spectra against the same call with numpy's: 100 times the worst relative
# difference measured on the eight units of test_driver_on_the_device, 2.55e-15 (DESIGN.md 8k has the record)
DRIVER_RTOL = 2.6e-13
# the routes of test_driver_routes_dosage_and_grm_mat, whose units were not part of that measurement: the difference
# above which an eigenvalue crossing the LAMBDA_DROP cut is the suspect
ROUTE_RTOL = 1e-9
_cache = {}


def gram_case(m, rows=60, seed=0):
    """A = diag(w) G' diag(v) G diag(w): ``rows`` random hard-call rows, minor allele frequencies spread over [0.005,
    0.5] on a log scale, w = dbeta(maf; 1, 25) -- about six decades on the diagonal."""
    key = (m, rows, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * m + seed)
        maf = np.exp(rng.uniform(np.log(0.005), np.log(0.5), m))
        G = rng.binomial(2, maf[None, :], size=(rows, m)).astype(np.float64)
        G[rng.integers(0, rows, m), np.arange(m)] += 1.0                  # every variant has a carrier
        v = rng.uniform(0.05, 0.25, rows)
        w = 25.0 * (1 - maf) ** 24
        A = (G * v[:, None]).T @ G
        A = 0.5 * (A + A.T) * w[:, None] * w[None, :]
        _cache[key] = np.ascontiguousarray(0.5 * (A + A.T))
    return _cache[key]


def scanner():
    import torch  # noqa: F401
    from conftest import scan_model
    from saigegds_amd._lib import Scanner
    return Scanner(scan_model("saige_model.npz", mac=0.0, maf=0.0, missing=1.0))


def mp_spectra(A, rho):
    """Eigenvalues of the closed-form matrices at 40 digits, built in mpmath from the double entries of A."""
    import mpmath as mp
    m = A.shape[0]
    re = np.minimum(rho, 0.999) if len(rho) > 1 else np.asarray(rho, dtype=np.float64)
    with mp.workdps(40):
        Am = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                Am[i, j] = mp.mpf(float(A[min(i, j), max(i, j)]))
        r = [mp.fsum(Am[i, j] for j in range(m)) for i in range(m)]
        c = mp.fsum(r)
        out = []
        for rk in list(re) + [None]:
            B = mp.matrix(m, m)
            if rk is not None:
                a = mp.sqrt(1 - mp.mpf(float(rk)))
                b = (mp.sqrt(1 - mp.mpf(float(rk)) + m * mp.mpf(float(rk))) - a) / m
            for i in range(m):
                for j in range(m):
                    B[i, j] = Am[i, j] - r[i] * r[j] / c if rk is None else a * a * Am[i, j] + a * b * (r[i] + r[j]) + b * b * c
            out.append(sorted(mp.eigsy(B, eigvals_only=True)))
        return out


def np_spectra(A, rho):
    from saigegds_amd.skato import skato_matrices
    return np.array([np.linalg.eigvalsh(B) for B in skato_matrices(A, rho)])


@pytest.mark.parametrize("m", [1, 2, 3, 15, 16, 17])
def test_kernel_against_40_digit_eigenvalues(m):
    import mpmath as mp
    A = gram_case(m)
    assert m < 15 or np.diag(A).max() / np.diag(A).min() > 1e3
    with scanner() as sc:
        lam, sw = sc.skato_spectra([A], RHO)
    assert lam[0].shape == (len(RHO) + 1, m) and sw.shape == (1, len(RHO) + 1) and np.all((sw >= 0) & (sw <= 30))
    assert np.all(np.diff(lam[0], axis=1) >= 0)
    ref = mp_spectra(A, RHO)
    worst = 0.0
    with mp.workdps(40):
        for g, r in zip(lam[0], ref):
            bound = 16 * m * EPS * max(abs(x) for x in r)
            for x, y in zip(g, r):
                d = abs(mp.mpf(float(x)) - y)
                assert d <= bound, (m, float(d), float(bound))
                if bound > 0:
                    worst = max(worst, float(d / bound))
    print(f"m = {m}: worst |dlam| / (16 m eps lam_max) = {worst:.3g}, sweeps {sw[0].tolist()}")


@pytest.mark.parametrize("m", [31, 32, 33, 63, 64, 65, 128, 129, 256])
def test_kernel_against_numpy(m):
    from saigegds_amd._lib import SKATO_MAX_M
    assert SKATO_MAX_M == 256
    A = gram_case(m, rows=400)
    with scanner() as sc:
        lam, sw = sc.skato_spectra([A], RHO)
    ref = np_spectra(A, RHO)
    bound = 2 * 16 * m * EPS * np.abs(ref).max(axis=1)
    ratio = np.abs(lam[0] - ref).max(axis=1) / bound
    print(f"m = {m}: worst |dlam| / (32 m eps lam_max) = {ratio.max():.3g}, sweeps {sw[0].tolist()}")
    assert np.all(ratio <= 1) and np.all((sw >= 1) & (sw <= 30)) and np.all(np.diff(lam[0], axis=1) >= 0)


@pytest.mark.parametrize("m", [17, 129])
def test_structured_matrices(m):
    rng = np.random.default_rng(m)
    bound = lambda lmax: 2 * 16 * m * EPS * lmax                                   # noqa: E731
    with scanner() as sc:
        # diagonal, the plain grid (0,): nothing to rotate, the sorted diagonal bit for bit
        d = rng.uniform(0.1, 10.0, m) * 10.0 ** rng.integers(-3, 4, m)
        lam, sw = sc.skato_spectra([np.diag(d)], (0,))
        assert np.array_equal(lam[0][0], np.sort(d)) and sw[0, 0] == 0
        # 11': one eigenvalue m, the rest 0
        lam, sw = sc.skato_spectra([np.ones((m, m))], (0,))
        assert abs(lam[0][0][-1] - m) <= bound(m) and np.all(np.abs(lam[0][0][:-1]) <= bound(m)) and 0 < sw[0, 0] <= 30
        # I: B_rho = R, eigenvalues 1 - rho (m - 1 times) and 1 - rho + m rho; W = I - 11' / m: one 0, the rest 1
        lam, sw = sc.skato_spectra([np.eye(m)], RHO)
        for k, rk in enumerate(np.minimum(RHO, 0.999)):
            top = 1 - rk + m * rk
            assert np.all(np.abs(lam[0][k][:-1] - (1 - rk)) <= bound(top)) and abs(lam[0][k][-1] - top) <= bound(top), (m, rk)
        assert abs(lam[0][-1][0]) <= bound(1) and np.all(np.abs(lam[0][-1][1:] - 1) <= bound(1))
        # rank-deficient: every column twice
        h = (m + 1) // 2
        G = rng.standard_normal((3 * m, h))
        G = np.concatenate([G, G[:, :m - h]], axis=1)
        A = G.T @ G
        A = 0.5 * (A + A.T)
        lam, sw = sc.skato_spectra([A], RHO)
        ref = np_spectra(A, RHO)
        assert np.all(np.abs(lam[0] - ref).max(axis=1) <= bound(np.abs(ref).max(axis=1))) and np.all((sw >= 1) & (sw <= 30))
        assert np.all(np.abs(lam[0][0][:m - h]) <= bound(ref[0].max()))
        # powers of two: the same bits, scaled
        A = gram_case(m, rows=200)
        lam, sw = sc.skato_spectra([A, A * 2.0 ** 200, A * 2.0 ** -200], RHO)
        assert np.all(np.isfinite(lam[0])) and np.array_equal(lam[1], lam[0] * 2.0 ** 200)
        assert np.array_equal(lam[2], lam[0] * 2.0 ** -200) and np.array_equal(sw[1], sw[0]) and np.array_equal(sw[2], sw[0])


def test_independence():
    sizes = [3, 17, 40, 70, 129, 16, 33, 1]
    others = [gram_case(k, rows=150, seed=5) for k in sizes]
    for m in (13, 65, 150):
        A = gram_case(m, rows=200, seed=9)
        with scanner() as sc:
            alone, sw = sc.skato_spectra([A], RHO)
            last, sw_l = sc.skato_spectra(others + [A], RHO)
            first, sw_f = sc.skato_spectra([A] + others[::-1], RHO)
            again, sw_a = sc.skato_spectra(others + [A], RHO)
            sub, sw_s = sc.skato_spectra([A], (0.04, 0.25, 1))               # the same grid values in another grid
            one, sw_1 = sc.skato_spectra([A], (0.25,))
        assert np.array_equal(last[-1], alone[0]) and np.array_equal(sw_l[-1], sw[0])
        assert np.array_equal(first[0], alone[0]) and np.array_equal(sw_f[0], sw[0])
        assert all(np.array_equal(x, y) for x, y in zip(last, again)) and np.array_equal(sw_l, sw_a)
        assert all(np.array_equal(x, y) for x, y in zip(last[:-1], first[:0:-1]))
        assert np.array_equal(sub[0], alone[0][[2, 4, 6, 7]]) and np.array_equal(one[0], alone[0][[4, 7]])


def test_errors_leave_the_handle_usable():
    from saigegds_amd._lib import SKATO_MAX_M, SgxError
    A, B, C_ = gram_case(17), gram_case(40, rows=100), gram_case(16)
    bad = B.copy()
    bad[3, 7] = bad[7, 3] = float("nan")
    with scanner() as sc:
        ok, sw_ok = sc.skato_spectra([A, B, C_], RHO)
        lam, sw = sc.skato_spectra([A, bad, C_], RHO)
        assert np.all(np.isnan(lam[1])) and np.all(sw[1] == -1)
        assert np.array_equal(lam[0], ok[0]) and np.array_equal(lam[2], ok[2]) and np.array_equal(sw[[0, 2]], sw_ok[[0, 2]])
        with pytest.raises(SgxError, match="at most") as ei:
            sc.skato_spectra([A, np.eye(SKATO_MAX_M + 1)], RHO)
        assert ei.value.code == -1
        for grid in ((), (0.5, 0.25), (0, 1.5)):
            with pytest.raises(SgxError) as ei:
                sc.skato_spectra([A], grid)
            assert ei.value.code == -1
        none, sw0 = sc.skato_spectra([], RHO)                             # n = 0 is legal
        assert none == [] and sw0.shape == (0, len(RHO) + 1)
        lam, sw = sc.skato_spectra([np.zeros((0, 0)), A], RHO)              # and so is an empty problem
        assert lam[0].shape == (len(RHO) + 1, 0) and np.all(sw[0] == 0) and np.array_equal(lam[1], ok[0])


def _hidden_factory():
    """A Scanner whose ``skato_spectra`` cannot be seen: the driver then takes numpy for every spectrum."""
    from saigegds_amd._lib import Scanner

    class NoSpectra(Scanner):
        @property
        def skato_spectra(self):
            raise AttributeError("skato_spectra")
    return NoSpectra


def test_driver_on_the_device():
    import torch  # noqa: F401
    from conftest import load_null_model
    from saigegds_amd import seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO
    path = os.path.join(GOLD, "grm1k_10k_snp.gds")
    mod = load_null_model("saige_model.npz")
    sizes = [1, 2, 5, 16, 17, 25, 33, 40]
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    units = [np.arange(a, a + k) + 1 for a, k in zip(starts, sizes)]
    dev = seqAssocGLMM_spaSKATO(path, mod, units, verbose=False)
    host = seqAssocGLMM_spaSKATO(path, mod, units, verbose=False, scanner_factory=_hidden_factory())
    skat = seqAssocGLMM_spaSKAT(path, mod, units, verbose=False)
    assert list(dev) == list(host) and (dev["n.var"] > 0).all()
    worst = 0.0
    for w in ("b1_1", "b1_25"):
        assert np.array_equal(host[f"pval.SKAT.{w}"], skat[f"pval.{w}"])          # the numpy route IS the SKAT driver's
        assert np.array_equal(dev[f"Q.{w}"], host[f"Q.{w}"]) and np.array_equal(dev[f"pval.burden.{w}"], host[f"pval.burden.{w}"])
        assert np.array_equal(dev[f"rho.min.{w}"], host[f"rho.min.{w}"])
        for c in ("pval.SKAT", "pval.burden", "pval"):
            a, b = dev[f"{c}.{w}"], host[f"{c}.{w}"]
            assert np.all(np.isfinite(a)) and np.all((a > 0) & (a <= 1))
            rel = np.abs(a - b) / b
            print(f"{c}.{w}: worst relative difference device / numpy {rel.max():.3g}")
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= DRIVER_RTOL), (c, w, rel)
    print(f"worst relative difference over the eight units: {worst:.3g}")


def test_driver_routes_dosage_and_grm_mat():
    import torch  # noqa: F401
    from conftest import load_null_model
    from saigegds_amd import seqAssocGLMM_spaSKATO
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    mod = load_null_model("saige_model.npz")
    ids = [str(s) for s in g["sample_id"]]
    codes = unpack_dosage_2bit(g["packed"][:60], 1000)
    units = [np.arange(1, 21), np.arange(21, 61)]
    # imputed dosages: the resident dosage block's SKAT step
    ds = GenotypeSource(ids, dosage=np.where(codes == 3, np.nan, codes * 0.5))
    dev = seqAssocGLMM_spaSKATO(ds, mod, units, wbeta=[1, 25], verbose=False)
    host = seqAssocGLMM_spaSKATO(ds, mod, units, wbeta=[1, 25], verbose=False, scanner_factory=_hidden_factory())
    assert list(dev) == list(host) and "n.iter" not in dev
    for c in ("pval", "pval.SKAT", "pval.burden"):
        assert np.all(np.isfinite(dev[c])) and np.all(np.abs(dev[c] - host[c]) <= ROUTE_RTOL * host[c]), c
    # an explicit GRM (the identity, as a dense pair): Phi^K, a column n.iter
    km = seqAssocGLMM_spaSKATO(os.path.join(GOLD, "grm1k_10k_snp.gds"), mod, units, wbeta=[1, 25], verbose=False,
                               grm_mat=(ids, np.eye(1000)))
    cols = list(km)
    assert cols[cols.index("n.var") + 1] == "n.iter" and cols[-5:] == ["pval", "pval.SKAT", "pval.burden", "rho.min", "Q"]
    assert np.all(km["n.iter"] >= 1) and np.all(np.isfinite(km["pval"])) and np.all((km["pval"] > 0) & (km["pval"] <= 1))
