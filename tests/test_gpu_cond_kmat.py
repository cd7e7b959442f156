"""sgx_cond_kmat_set and sgx_cond_kmat_2bit on the device, through the C ABI's ctypes binding.

The references, the case table and the recorded tolerance are in tests/cond_kmat_ref.py (built on tests/skat_kmat_ref.py).

* the set and every row against sgx_skat_kmat_2bit on the units (c_1 .. c_C) and (c_1 .. c_C, j): bit for bit;
* against the long-double reference at tol = 1e-12, maxiter = 500: scaled_error <= PHI_TOL = 5.55e-7, the project's bound
  for Phi^K (10 x the float64 reference's own discrepancy);
* a row's bits do not depend on the other rows, their order, or a set installed in between;
* tau[1] = 0: tau[0] * var_ratio * (var, cov) against sgx_cond_2bit at 1e-10 relative, every column in 0 or 1 steps;
* non-finite tables; the SGX_EINVAL list.
"""
import numpy as np
import pytest

import cond_kmat_ref as CK
import skat_kmat_ref as M

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in CK.CASES]
_dev = {}


def operator(c):
    from saigegds_amd._lib import ExplicitGrmOperator
    return ExplicitGrmOperator(csr=c["csr"]) if c["storage"] == "csr" else ExplicitGrmOperator(c["K"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def units_of(n_cond, rows):
    """The units (c_1 .. c_C, j) of the scanned rows `rows` (indices into packed) as one CSR, the set as unit 0."""
    vi = [np.arange(n_cond)] + [np.concatenate([np.arange(n_cond), [j]]) for j in rows]
    return np.concatenate([[0], np.cumsum([v.size for v in vi])]).astype(np.int64), np.concatenate(vi).astype(np.int32)


def dev(name):
    """One device run per case, shared by checks 1 to 3: the new entries and sgx_skat_kmat_2bit on the units."""
    if name in _dev:
        return _dev[name]
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = CK.make_case(name)
    nc, packed, lut = c["n_cond"], c["packed"], c["lut"]
    up, vi = units_of(nc, range(nc, packed.shape[0]))
    with Scanner(c["sm"]) as sc, operator(c) as op:
        st = sc.cond_kmat_set(op, packed[:nc], lut[:nc], c["w"], c["tau"], M.MAXITER, M.TOL_SOLVE)
        rows = sc.cond_kmat(op, packed[nc:], lut[nc:])
        unit = sc.skat_kmat(op, packed, up, vi, lut[vi], c["w"], c["tau"], maxiter=M.MAXITER, tol=M.TOL_SOLVE)
    _dev[name] = (st, rows, unit, up)
    return _dev[name]


@pytest.mark.parametrize("name", NAMES)
def test_1_2_the_set_and_every_row_equal_skat_kmat_on_their_units(name):
    c = CK.make_case(name)
    nc = c["n_cond"]
    (S_C, phi_cc, it_c), (score, var, cov, it), (us, uc, ui), up = dev(name)
    assert same_bits(S_C, us[:nc]) and same_bits(phi_cc, uc[0]) and np.array_equal(it_c, ui[:nc])
    assert score.shape == var.shape == it.shape == (c["rows"],) and cov.shape == (c["rows"], nc)
    for j in range(c["rows"]):
        u, e = uc[1 + j], int(up[2 + j]) - 1                 # the unit's matrix, the row's entry
        assert same_bits(score[j], us[e]) and it[j] == ui[e], f"{name} row {j}"
        assert same_bits(var[j], u[nc, nc]), f"{name} row {j}: var {var[j]!r} != {u[nc, nc]!r}"
        assert same_bits(cov[j], u[nc, :nc]), f"{name} row {j}: cov"


@pytest.mark.parametrize("name", NAMES)
def test_3_against_the_long_double_reference(name):
    ref = CK.case_ref(name, "ld")
    (S_C, phi_cc, it_c), (score, var, cov, it), _, _ = dev(name)
    assert int(max(it.max(), it_c.max())) < M.MAXITER
    worst = M.scaled_error(phi_cc, ref["Phi_CC"])
    for j, u in enumerate(ref["units"]):
        worst = max(worst, M.scaled_error(CK.unit_matrix(phi_cc, cov[j], var[j]), u))
    print(f"{name}: Phi^K off the long-double reference by {worst:.3g} (bound {M.PHI_TOL:.3g}), iters <= {int(it.max())}")
    assert worst <= M.PHI_TOL, name


def test_4_a_rows_bits_do_not_depend_on_the_call():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    name = "n1003_k3_c7_csr"
    c = CK.make_case(name)
    nc, packed, lut = c["n_cond"], c["packed"], c["lut"]
    _, (score, var, cov, it), _, _ = dev(name)
    rows, tabs = packed[nc:], lut[nc:]
    perm = np.random.default_rng(4).permutation(c["rows"])
    sub = np.array([129, 3, 64, 70])
    with Scanner(c["sm"]) as sc, operator(c) as op:
        sc.cond_kmat_set(op, packed[:nc], lut[:nc], c["w"], c["tau"], M.MAXITER, M.TOL_SOLVE)
        p = sc.cond_kmat(op, rows[perm], tabs[perm])
        # another set (three of the scanned rows, another tau) installed and replaced in between
        sc.cond_kmat_set(op, rows[10:13], tabs[10:13], c["w"], [1.3, 0.2], M.MAXITER, 1e-6)
        other = sc.cond_kmat(op, rows[:5], tabs[:5])
        sc.cond_kmat_set(op, packed[:nc], lut[:nc], c["w"], c["tau"], M.MAXITER, M.TOL_SOLVE)
        s = sc.cond_kmat(op, rows[sub], tabs[sub])
    assert other[2].shape == (5, 3)
    for got, idx in ((p, perm), (s, sub)):
        assert same_bits(got[0], score[idx]) and same_bits(got[1], var[idx]) and same_bits(got[2], cov[idx])
        assert np.array_equal(got[3], it[idx])


@pytest.mark.parametrize("name", ["n61_k3_c16_dense", "n1003_k3_c7_csr", "n4099_k5_c7_csr"])
def test_5_tau1_zero_is_the_variance_ratio_form(name):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = CK.make_case(name)
    sm, nc, packed, lut = c["sm"], c["n_cond"], c["packed"], c["lut"]
    mu2 = np.ones(sm.n) if sm.quant else np.ascontiguousarray(sm.mu2)
    t0 = float(c["tau"][0])
    with Scanner(sm) as sc, operator(c) as op:
        S_C, phi_cc, it_c = sc.cond_kmat_set(op, packed[:nc], lut[:nc], mu2, [t0, 0.0], M.MAXITER, M.TOL_SOLVE)
        score, var, cov, it = sc.cond_kmat(op, packed[nc:], lut[nc:])
        s2_c, phi2 = sc.cond_set(packed[:nc], lut[:nc])
        s2, var2, cov2 = sc.cond_2bit(packed[nc:], lut[nc:])
    assert set(np.unique(np.concatenate([it, it_c])).tolist()) <= {0, 1}
    f = t0 * sm.var_ratio
    sd, sd_c = np.sqrt(np.maximum(var2, 0)), np.sqrt(np.maximum(np.diag(phi2), 0))
    scale = lambda a, b: np.where(a[:, None] * b[None, :] > 0, a[:, None] * b[None, :], 1.0)      # noqa: E731  (variance 0: a monomorphic row, exact zeros)
    e_v = np.abs(f * var - var2) / np.where(var2 > 0, var2, 1.0)
    e_c = np.abs(f * cov - cov2) / scale(sd, sd_c)
    e_cc = np.abs(f * phi_cc - phi2) / scale(sd_c, sd_c)
    print(f"{name}: tau1 = 0 against sgx_cond_2bit: var {e_v.max():.3g}, cov {e_c.max():.3g}, Phi_CC {e_cc.max():.3g}")
    assert e_v.max() <= 1e-10 and e_c.max() <= 1e-10 and e_cc.max() <= 1e-10


def test_6_non_finite_tables_poison_their_own_rows_only():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = CK.make_case("n61_k1_c1_csr")                        # 65 scanned rows
    nc, packed, lut = c["n_cond"], c["packed"], c["lut"]
    rows, tabs = packed[nc:], lut[nc:].copy()
    bad = np.array([7, 64])
    tabs[7, 3], tabs[64, 0] = np.nan, np.inf
    keep = np.setdiff1d(np.arange(65), bad)
    with Scanner(c["sm"]) as sc, operator(c) as op:
        sc.cond_kmat_set(op, packed[:nc], lut[:nc], c["w"], c["tau"], M.MAXITER, M.TOL_SOLVE)
        a = sc.cond_kmat(op, rows, tabs)
        b = sc.cond_kmat(op, rows[keep], tabs[keep])
    assert not np.isfinite(a[0][bad]).any() and not np.isfinite(a[1][bad]).any() and not np.isfinite(a[2][bad]).any()
    assert np.all(a[3][bad] == 0)
    for x, y in zip(a[:3], b[:3]):
        assert same_bits(x[keep], y)
    assert np.array_equal(a[3][keep], b[3]) and np.isfinite(b[1]).all()


def test_7_errors_launch_nothing_and_leave_the_handles_usable():
    import torch  # noqa: F401
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner, COND_MAX
    name = "n61_k1_c1_csr"
    c = CK.make_case(name)
    sm, packed, lut, w, tau = c["sm"], c["packed"], c["lut"], c["w"], c["tau"]
    _, good, _, _ = dev(name)
    with Scanner(sm) as sc, operator(c) as op, ExplicitGrmOperator(np.eye(60)) as op60, ExplicitGrmOperator(np.eye(61)) as op61:
        L, h = sc._L, sc._h
        vr_c, vr_cc = sc.cond_set(packed[:1], lut[:1])                 # the variance-ratio set, installed beforehand
        vr = sc.cond_2bit(packed[1:], lut[1:])
        s_c, cc, it_c = np.zeros(COND_MAX + 1), np.zeros((COND_MAX + 1) ** 2), np.zeros(COND_MAX + 1, dtype=np.int32)
        score, var, cov, it = np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int32)
        big = np.ascontiguousarray(np.tile(packed[:1], (COND_MAX + 1, 1)))
        big_lut = np.ascontiguousarray(np.tile(lut[:1], (COND_MAX + 1, 1)))

        def cset(n=1, **kw):
            a = dict(h=h, km=op._h, packed=packed.ctypes.data, bpv=packed.shape[1], lut=lut.ctypes.data, w=w.ctypes.data,
                     tau=tau.ctypes.data, s=s_c.ctypes.data, cc=cc.ctypes.data)
            a.update(kw)
            return L.sgx_cond_kmat_set(a["h"], a["km"], a["packed"], a["bpv"], n, a["lut"], a["w"], a["tau"], 500, 1e-12,
                                       a["s"], a["cc"], it_c.ctypes.data)

        def scan(n=1, **kw):
            a = dict(h=h, km=op._h, packed=packed[1:].ctypes.data, bpv=packed.shape[1], lut=lut[1:].ctypes.data,
                     s=score.ctypes.data, v=var.ctypes.data, c=cov.ctypes.data)
            a.update(kw)
            return L.sgx_cond_kmat_2bit(a["h"], a["km"], a["packed"], a["bpv"], n, a["lut"], a["s"], a["v"], a["c"], it.ctypes.data)

        assert scan() == -1                                            # no set installed
        for k in ("packed", "lut", "w", "tau", "s", "cc", "km", "h"):
            assert cset(**{k: None}) == -1, k
        assert cset(n=COND_MAX + 1, packed=big.ctypes.data, lut=big_lut.ctypes.data) == -1
        assert cset(km=op60._h) == -1                                  # another sample count
        assert cset(bpv=(sm.n + 3) // 4 - 1) == -1
        for bad_w in (0.0, -1.0, np.nan, np.inf):
            w2 = w.copy()
            w2[7] = bad_w
            assert cset(w=w2.ctypes.data) == -1, bad_w
        for bad_tau in ([0.0, 0.5], [-1.0, 0.5], [1.0, -0.1], [np.nan, 0.1]):
            t2 = np.array(bad_tau)
            assert cset(tau=t2.ctypes.data) == -1, bad_tau
        assert scan() == -1                                            # still no set
        assert np.all(s_c == 0) and np.all(cc == 0) and np.all(it_c == 0)

        S_C, phi_cc, _ = sc.cond_kmat_set(op, packed[:1], lut[:1], w, tau, M.MAXITER, M.TOL_SOLVE)
        for k in ("packed", "lut", "s", "v", "c", "km", "h"):
            assert scan(**{k: None}) == -1, k
        assert scan(km=op61._h) == -1                                  # not the set's matrix
        assert scan(km=op60._h) == -1
        assert scan(bpv=(sm.n + 3) // 4 - 1) == -1
        assert cset(w=None) == -1                                      # a refused set leaves the installed one
        assert np.all(score == 0) and np.all(var == 0) and np.all(cov == 0) and np.all(it == 0)
        assert scan(n=0) == 0 and np.all(score == 0)
        again = sc.cond_kmat(op, packed[1:], lut[1:])
        for x, y in zip(again, good):
            assert same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)
        # the variance-ratio set is where it was; clearing one set leaves the other
        vr2 = sc.cond_2bit(packed[1:], lut[1:])
        assert all(same_bits(x, y) for x, y in zip(vr, vr2))
        sc.cond_kmat_set(op, packed[:0], lut[:0], w, tau)
        assert scan() == -1
        assert all(same_bits(x, y) for x, y in zip(vr, sc.cond_2bit(packed[1:], lut[1:])))
        sc.cond_kmat_set(op, packed[:1], lut[:1], w, tau, M.MAXITER, M.TOL_SOLVE)
        sc.cond_set(packed[:0], lut[:0])
        again = sc.cond_kmat(op, packed[1:], lut[1:])
        assert same_bits(again[1], good[1]) and same_bits(again[2], good[2])


def test_8_host_rows_in_chunks_of_more_than_one_solve():
    """sgx_cond_kmat_2bit sends its rows up in chunks of pipe_mb MiB at the device stride 4 ceil(N / 16): 17 504 bytes at
    N = 70 001, so pipe_mb = 2 is 119 rows a chunk -- more than the SGX_GRM_MAX_RHS = 64 columns of a solve and not a
    multiple of them, so that a chunk is two solves (64 + 55) whose second reads the rows and tables from row 64 on.
    120 rows (a chunk and one row) and 245 (two chunks and a tail of 7, not a multiple of 16), K = 2, C = 2, on a GRM of
    pairs: the bits of the one-chunk call."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = M.chunk_case(2 + 245, 43)
    packed, lut = c["packed"], c["lut"]
    assert (2 << 20) // (4 * ((70001 + 15) // 16)) == 119
    with Scanner(c["sm"]) as sc, operator(c) as op:
        sc.cond_kmat_set(op, packed[2:4], lut[2:4], c["w"], c["tau"], M.MAXITER, M.TOL_SOLVE)
        rows, tabs = np.delete(packed, [2, 3], axis=0), np.delete(lut, [2, 3], axis=0)
        try:
            for m in (120, 245):
                got = {}
                for pipe_mb in (0, 2):
                    sc.set_option("pipe_mb", pipe_mb)
                    got[pipe_mb] = sc.cond_kmat(op, rows[:m], tabs[:m])
                assert np.isfinite(got[0][1]).sum() >= m - 2 and got[0][2].shape == (m, 2)
                for k in range(3):
                    assert got[0][k].tobytes() == got[2][k].tobytes(), (m, k)
                assert np.array_equal(got[0][3], got[2][3]), m
        finally:
            sc.set_option("pipe_mb", 0)
