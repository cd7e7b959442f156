"""sgx_cond_set / sgx_cond_2bit(_dev) and seqAssocGLMM_SPA_cond on the device: the rectangular kernel against the
long-double reference of tests/cond_ref.py, the identities that tie it to sgx_skat_2bit and to the pinned scan,
determinism, non-finite tables, the error paths, and the driver against its run with the numpy stand-in scanner of
tests/test_cond.py.  Models and rows as in tests/test_gpu_skat.py: the golden models at N = 1000, synth_null_model
otherwise; hard calls with 1 % missing, every 7th row alt-major.  The first NC rows of a case are the conditioning set."""
import os

import numpy as np
import pytest

import cond_ref as CR
import skat_ref as R
from test_cond import golden_rows
from test_gpu_skat import _flat, _model

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NC = 8
WG_ROWS = 256             # COND_WG_ROWS of kern_cond.h: the rows one workgroup owns
_cache = {}


def _case(n):
    """Per N, made once: model, NC conditioning rows + WG_ROWS + 1 scanned rows, tables, the long-double reference."""
    if n not in _cache:
        from saigegds_amd.gds import pack_dosage_2bit
        sm = _model(n)
        codes = R.hard_calls(n, NC + WG_ROWS + 1, 17 + n)
        packed, lut = pack_dosage_2bit(codes), R.tables(codes)
        ref = CR.cond_ref(sm, packed[NC:], lut[NC:], packed[:NC], lut[:NC])
        _cache[n] = (sm, packed[NC:], lut[NC:], packed[:NC], lut[:NC], ref)
    return _cache[n]


def check(score, var, cov, ref, rows, what):
    """The bounds of check() in tests/test_gpu_skat.py: |dS_j| <= 1e-10 |S_j| + 1e-12 sqrt(Phi_jj),
    |dPhi_jl| <= 1e-10 sqrt(Phi_jj Phi_ll) for l = j and l in the conditioning set (derived there, not measured)."""
    from conftest import REL_TOL, Z_FLOOR
    S, v, cv = ref["S"][rows], ref["var"][rows], ref["cov"][rows]
    sd, sdc = np.sqrt(v), np.sqrt(np.diag(ref["Phi_CC"]))
    assert score.shape == S.shape and var.shape == v.shape and cov.shape == cv.shape, what
    assert np.all(np.isfinite(score)) and np.all(np.isfinite(var)) and np.all(np.isfinite(cov)), what
    e_s = np.abs(score - S) / (REL_TOL * np.abs(S) + Z_FLOOR * sd)
    e_v = np.abs(var - v) / (REL_TOL * v)
    e_c = np.abs(cov - cv) / (REL_TOL * sd[:, None] * sdc[None, :])
    print(f"{what}: S off by {float(e_s.max()):.3g} x tolerance, Phi_jj by {float(e_v.max()):.3g} x, Phi_jc by {float(e_c.max()):.3g} x")
    assert float(e_s.max()) <= 1.0 and float(e_v.max()) <= 1.0 and float(e_c.max()) <= 1.0, what


@pytest.mark.parametrize("m", [1, 15, 16, 17, 40, WG_ROWS + 1])
@pytest.mark.parametrize("n", [1000, 70001])
def test_1_kernel_against_the_reference(n, m):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, packed, lut, pc, lc, ref = _case(n)
    with Scanner(sm) as sc:
        s_c, phi_cc = sc.cond_set(pc, lc)
        score, var, cov = sc.cond_2bit(packed[:m], lut[:m])
    check(score, var, cov, ref, slice(0, m), f"N={n} m={m}")
    R_cc = np.asarray(ref["Phi_CC"], dtype=np.float64)
    assert np.all(np.abs(phi_cc - R_cc) <= 1e-10 * np.sqrt(np.outer(np.diag(R_cc), np.diag(R_cc))))
    assert np.array_equal(phi_cc, phi_cc.T)


@pytest.mark.parametrize("k,c", [(3, 1), (3, 8), (3, 9), (3, 10), (8, 16), (16, 16)])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_2_column_tile_edges(trait, k, c):
    """2K + 1 + C = 8, 15, 16, 17, 33, 49 columns of B: inside one tile, one short of it, exactly one, one over, one
    over two, one over three."""
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 1000, 17
    sm = _flat(synth.synth_null_model(n, trait, 0.2, n_cov=k, seed=20260 + k))
    assert sm.k == k
    codes = R.hard_calls(n, c + m, 5 + k + c)
    packed, lut = pack_dosage_2bit(codes), R.tables(codes)
    ref = CR.cond_ref(sm, packed[c:], lut[c:], packed[:c], lut[:c])
    with Scanner(sm) as sc:
        sc.cond_set(packed[:c], lut[:c])
        score, var, cov = sc.cond_2bit(packed[c:], lut[c:])
    check(score, var, cov, ref, slice(0, m), f"{trait} K={k} C={c}")


def test_3_cond_set_equals_skat_2bit():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    for n in (1000, 70001):
        sm, _, _, pc, lc, _ = _case(n)
        with Scanner(sm) as sc:
            s_c, phi_cc = sc.cond_set(pc, lc)
            s, covs = sc.skat_2bit(pc, [0, NC], np.arange(NC), lc)
        assert s_c.tobytes() == s.tobytes() and phi_cc.tobytes() == covs[0].tobytes(), n


def test_4_ties_to_the_square_kernel():
    """cov[j][c] and var[j] against skat_2bit on the unit {j} + C, within the bound of test 1."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, packed, lut, pc, lc, _ = _case(70001)
    m = 40
    allp, alll = np.concatenate([pc, packed[:m]]), np.concatenate([lc, lut[:m]])
    idx = np.concatenate([np.concatenate([[NC + j], np.arange(NC)]) for j in range(m)])
    ptr = np.arange(0, (m + 1) * (NC + 1), NC + 1)
    with Scanner(sm) as sc:
        sc.cond_set(pc, lc)
        score, var, cov = sc.cond_2bit(packed[:m], lut[:m])
        s2, covs = sc.skat_2bit(allp, ptr, idx, alll[idx])
    worst = 0.0
    for j in range(m):
        phi = covs[j]
        sd = np.sqrt(np.diag(phi))
        e = np.abs(np.concatenate([[var[j]], cov[j]]) - phi[0]) / (1e-10 * sd[0] * sd)
        worst = max(worst, float(e.max()))
        assert abs(score[j] - s2[ptr[j]]) <= 1e-10 * abs(s2[ptr[j]]) + 1e-12 * sd[0]
    print("largest difference to the square kernel, in units of the tolerance:", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_5_ties_to_the_pinned_scan(trait):
    """chdtrc(1, score^2 / var) = the pval_noadj of Scanner.scan_2bit on the same rows, as test_3 of test_gpu_skat."""
    import torch  # noqa: F401
    from scipy.special import chdtrc
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:200], 1000)
    ok = codes != 3
    s, nn = np.where(ok, codes, 0).sum(axis=1), ok.sum(axis=1)
    pick = np.flatnonzero(np.minimum(s, 2 * nn - s) > 0)[:64 + 3]
    assert pick.size == 67
    packed = np.ascontiguousarray(g["packed"][pick])
    lut = R.tables(codes[pick])
    sm = _model(1000, trait)
    with Scanner(sm) as sc:
        out, valid = sc.scan_2bit(packed[3:])
        sc.cond_set(packed[:3], lut[:3])
        score, var, _ = sc.cond_2bit(packed[3:], lut[3:])
    assert valid.all()
    p = chdtrc(1.0, score ** 2 / var)
    ref = out[:, 5 if sm.quant else 6]
    err = np.abs(p - ref) / ref
    print(trait, "largest relative difference to the scan's pval_noadj", err.max())
    assert np.all(err <= 1e-10)


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_6_the_conditional_test_is_the_scan_of_the_residual_row(trait):
    """x = G_j - sum_c b_c G_c, b = Phi_CC^-1 Phi_Cj, shifted and scaled into (0, 1) (the intercept absorbs the shift,
    the chi-square is scale-free), scanned with scan_f64 at thresholds 0 / 0 / 1: qchisq(p.norm) = T^2 / V of
    cond_tests with d = 1.  40 golden rows, C = 3; rows the set explains to more than 90 % may be skipped (at most 4)."""
    import torch  # noqa: F401
    from scipy.special import chdtri
    from saigegds_amd._lib import Scanner
    from saigegds_amd.cond import cond_tests
    packed, codes, lut = golden_rows(43)
    sm = _model(1000, trait)
    ref = CR.cond_ref(sm, packed[3:], lut[3:], packed[:3], lut[:3])
    use = np.flatnonzero(1 - np.asarray(ref["V"] / ref["var"], dtype=np.float64) <= 0.9)
    assert use.size >= 36                                  # checked on the host, before anything runs on the device
    with Scanner(sm) as sc:
        s_c, phi_cc = sc.cond_set(packed[:3], lut[:3])
        score, var, cov = sc.cond_2bit(packed[3:], lut[3:])
        G = np.take_along_axis(lut, codes.astype(np.int64), axis=1)            # imputed, flipped dosages [43, N]
        b = np.linalg.solve(phi_cc, cov.T).T                                   # [40, 3]
        x = G[3:] - b @ G[:3]
        lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
        x = 0.01 + 0.98 * (x - lo) / (hi - lo)
        out, valid = sc.scan_f64(x[use])
    assert valid.all()
    beta, se, p = cond_tests(score, var, cov, s_c, phi_cc)
    chi = (beta[use] / se[use]) ** 2                                           # (T / V)^2 V = T^2 / V
    refchi = chdtri(1.0, out[:, 5 if sm.quant else 6])
    err = np.abs(chi - refchi) / refchi
    print(trait, "rows used", use.size, "largest relative difference to the scan of the residual row", err.max())
    assert np.all(err <= 1e-9)


def test_7_determinism():
    import torch
    from saigegds_amd._lib import Scanner
    sm, packed, lut, pc, lc, _ = _case(70001)
    m = 40
    with Scanner(sm) as sc:
        sc.cond_set(pc, lc)
        a = sc.cond_2bit(packed[:m], lut[:m])
        b = sc.cond_2bit(packed[:m], lut[:m])
        first = sc.cond_2bit(packed[:1], lut[:1])
        last = sc.cond_2bit(packed[m - 1:m], lut[m - 1:m])
        big = sc.cond_2bit(packed, lut)                                        # WG_ROWS + 1 rows
        sc.set_option("pipe_mb", 1)                                            # 59 rows a chunk at this N
        cut = sc.cond_2bit(packed, lut)
        sc.set_option("pipe_mb", 0)
        # the device entry
        stride = sc.row_stride()
        host = np.zeros((m, stride), dtype=np.uint8)
        host[:, :packed.shape[1]] = packed[:m]
        rows, tl = torch.from_numpy(host).cuda(), torch.from_numpy(lut[:m].copy()).cuda()
        s, v = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
        cv = torch.empty((m, NC), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sc.cond_2bit_dev(rows.data_ptr(), stride, m, tl.data_ptr(), s.data_ptr(), v.data_ptr(), cv.data_ptr())
        sc.sync()
        dev = (s.cpu().numpy(), v.cpu().numpy(), cv.cpu().numpy())
    for k in range(3):
        assert a[k].tobytes() == b[k].tobytes(), "twice"
        assert a[k][:1].tobytes() == first[k].tobytes(), "first row alone"
        assert a[k][m - 1:].tobytes() == last[k].tobytes(), "last row alone"
        assert a[k].tobytes() == big[k][:m].tobytes(), "among more rows"
        assert big[k].tobytes() == cut[k].tobytes(), "pipe_mb = 1"
        assert a[k].tobytes() == dev[k].tobytes(), "device entry"


def test_8_non_finite_table():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, packed, lut, pc, lc, _ = _case(1000)
    m = 40
    bad = lut[:m].copy()
    bad[5, 1] = np.nan
    bad[21, 3] = np.inf
    with Scanner(sm) as sc:
        sc.cond_set(pc, lc)
        good = sc.cond_2bit(packed[:m], lut[:m])
        got = sc.cond_2bit(packed[:m], bad)
    others = np.setdiff1d(np.arange(m), [5, 21])
    for k in range(3):
        assert not np.isfinite(got[k][5]).any() and not np.isfinite(got[k][21]).any()
        assert got[k][others].tobytes() == good[k][others].tobytes()


def test_9_errors_leave_the_handle_usable():
    import torch
    from saigegds_amd import _lib
    from saigegds_amd._lib import COND_MAX, Scanner
    L = _lib.load()
    sm, packed, lut, pc, lc, ref = _case(1000)
    m, bpv = 4, packed.shape[1]
    pk, lt = np.ascontiguousarray(packed[:m]), np.ascontiguousarray(lut[:m])
    s, v, cv = np.zeros(m), np.zeros(m), np.zeros(m * NC)
    sC, cC = np.zeros(COND_MAX + 1), np.zeros((COND_MAX + 1) ** 2)
    with Scanner(sm) as sc:
        h = sc._h

        def good():
            score, var, cov = sc.cond_2bit(pk, lt)
            check(score, var, cov, ref, slice(0, m), "after an error")
        # no set installed
        assert L.sgx_cond_2bit(h, pk.ctypes.data, bpv, m, lt.ctypes.data, s.ctypes.data, v.ctypes.data, cv.ctypes.data) == -1
        assert b"no conditioning set" in L.sgx_last_error()
        sc.cond_set(pc, lc)
        good()
        # sgx_cond_set
        big = np.zeros((COND_MAX + 1, bpv), dtype=np.uint8)
        bigl = np.tile(lc[:1], (COND_MAX + 1, 1))
        assert L.sgx_cond_set(h, big.ctypes.data, bpv, COND_MAX + 1, bigl.ctypes.data, sC.ctypes.data, cC.ctypes.data) == -1
        assert b"at most" in L.sgx_last_error()
        good()
        for args in ((None, bpv, NC, lc.ctypes.data, sC.ctypes.data, cC.ctypes.data),
                     (pc.ctypes.data, bpv, NC, None, sC.ctypes.data, cC.ctypes.data),
                     (pc.ctypes.data, bpv, NC, lc.ctypes.data, None, cC.ctypes.data),
                     (pc.ctypes.data, bpv, NC, lc.ctypes.data, sC.ctypes.data, None),
                     (pc.ctypes.data, bpv - 1, NC, lc.ctypes.data, sC.ctypes.data, cC.ctypes.data)):
            assert L.sgx_cond_set(h, *args) == -1
            good()
        # sgx_cond_2bit
        for args in ((None, bpv, m, lt.ctypes.data, s.ctypes.data, v.ctypes.data, cv.ctypes.data),
                     (pk.ctypes.data, bpv, m, None, s.ctypes.data, v.ctypes.data, cv.ctypes.data),
                     (pk.ctypes.data, bpv, m, lt.ctypes.data, None, v.ctypes.data, cv.ctypes.data),
                     (pk.ctypes.data, bpv, m, lt.ctypes.data, s.ctypes.data, None, cv.ctypes.data),
                     (pk.ctypes.data, bpv, m, lt.ctypes.data, s.ctypes.data, v.ctypes.data, None),
                     (pk.ctypes.data, bpv - 1, m, lt.ctypes.data, s.ctypes.data, v.ctypes.data, cv.ctypes.data)):
            assert L.sgx_cond_2bit(h, *args) == -1
            good()
        assert L.sgx_cond_2bit(h, None, bpv, 0, None, None, None, None) == 0           # no rows: nothing to do
        # sgx_cond_2bit_dev: NULL, stride, alignment
        stride = sc.row_stride()
        host = np.zeros((m + 1, stride), dtype=np.uint8)
        host[:m, :bpv] = pk
        rows, tl = torch.from_numpy(host).cuda(), torch.from_numpy(lt).cuda()
        ds, dv = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
        dc = torch.empty((m, NC), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ok = (rows.data_ptr(), stride, m, tl.data_ptr(), ds.data_ptr(), dv.data_ptr(), dc.data_ptr())
        for i, val in ((0, None), (3, None), (4, None), (5, None), (6, None), (1, stride - 64), (1, stride + 32), (0, rows.data_ptr() + 8)):
            args = list(ok)
            args[i] = val
            assert L.sgx_cond_2bit_dev(h, *args) == -1, (i, val)
            good()
        assert L.sgx_cond_2bit_dev(h, None, stride, 0, None, None, None, None) == 0
        sc.cond_2bit_dev(*ok)
        sc.sync()
        check(ds.cpu().numpy(), dv.cpu().numpy(), dc.cpu().numpy(), ref, slice(0, m), "device entry after the errors")
        # clearing the set
        sc.cond_set(np.zeros((0, bpv), dtype=np.uint8), np.zeros((0, 4)))
        assert L.sgx_cond_2bit(h, pk.ctypes.data, bpv, m, lt.ctypes.data, s.ctypes.data, v.ctypes.data, cv.ctypes.data) == -1
        sc.cond_set(pc, lc)
        good()


def test_10_driver_end_to_end():
    """grm1k_10k_snp.gds, first 2 000 variants given 2 of them: against the driver's run with the numpy stand-in
    scanner, and its scan columns against seqAssocGLMM_SPA."""
    import torch  # noqa: F401
    from conftest import assert_table_close, load_null_model
    from saigegds_amd import GenotypeSource, seqAssocGLMM_SPA, seqAssocGLMM_SPA_cond
    from saigegds_amd.gds import GdsFile
    from test_cond import ref_cond_scanner_factory
    f = GdsFile(os.path.join(GOLD, "grm1k_10k_snp.gds"))
    src = GenotypeSource(f.sample_id(), packed=f.dosage_alt_packed_range(0, 2000), variant_id=np.asarray(f.read("variant.id"))[:2000])
    mod = load_null_model("saige_model.npz")
    plain = seqAssocGLMM_SPA(src, mod, verbose=False)
    lead = np.argsort(plain["pval"])[:40]
    cond = [plain["id"][lead[0]], plain["id"][lead[7]]]
    got = seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False)
    ref = seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, scanner_factory=ref_cond_scanner_factory())
    assert list(got.keys()) == list(ref.keys()) == list(plain.keys()) + ["beta.cond", "SE.cond", "pval.cond"]
    for c in ("id", "pos", "num", "converged"):
        assert np.array_equal(got[c], plain[c]) and np.array_equal(got[c], ref[c]), c
    # the scan columns: the project's parity rule (integer columns exact, the rest within 1e-10)
    tab = lambda a: np.stack([np.asarray(a[c], dtype=np.float64) for c in ("AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged")], axis=1)  # noqa: E731
    ones = np.ones(len(got["id"]), dtype=np.uint8)
    assert_table_close(tab(got), ones, tab(plain), ones, what="scan columns against seqAssocGLMM_SPA")
    # The conditional columns against the stand-in's.  Both sides carry S and Phi to 1e-10 (of sqrt(Phi_jj Phi_ll)), and
    # the SPA factors d_j move with the scan's p-values (1e-10).  V = Phi_jj (1 - R^2) and T lose a factor 1 / (1 - R^2)
    # of that, and a chi-square z^2 turns its own relative error into (z^2 / 2 + 1) times as much of its p-value: the
    # bound 1e-8 leaves a factor 100 for the two together.
    k = np.isin(got["id"], cond)
    assert k.sum() == 2
    for c in ("beta.cond", "SE.cond", "pval.cond"):
        assert np.isnan(got[c][k]).all() and np.isnan(ref[c][k]).all(), c
        assert np.array_equal(np.isnan(got[c]), np.isnan(ref[c])), c
        assert np.isfinite(got[c][~k]).mean() > 0.99
    f = np.isfinite(ref["pval.cond"])
    assert np.all(np.abs(got["SE.cond"][f] - ref["SE.cond"][f]) <= 1e-8 * ref["SE.cond"][f])
    assert np.all(np.abs(got["beta.cond"][f] - ref["beta.cond"][f]) <= 1e-8 * np.abs(ref["beta.cond"][f]) + 1e-10 * ref["SE.cond"][f])
    assert np.all(np.abs(got["pval.cond"][f] - ref["pval.cond"][f]) <= 1e-8 * ref["pval.cond"][f])
