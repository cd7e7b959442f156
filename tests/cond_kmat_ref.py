"""Reference of sgx_cond_kmat_set / sgx_cond_kmat_2bit -- TEST INFRASTRUCTURE ONLY.

Built on tests/skat_kmat_ref.py: the conditional scan's ``Phi^K`` of row j is that module's ``Phi^K`` of the unit
``(c_1 .. c_C, j)``, so the two forms there (float64 CG with the device loop's stopping rule, long-double direct solve)
serve here with the set's rows in front.  The case table of tests/test_gpu_cond_kmat.py, the stand-in scanner of the
driver tests and the recorded tolerances are here too.

Recorded on the CPU (tests/test_cond_kmat_ref.py prints them):

    float64 CG against long double at tol = 1e-12, scaled as skat_kmat_ref.scaled_error, over the case table below:
    at most 5.46e-8 (n61_k1_c1_csr; 6e-16 .. 5e-8 over the cases), inside skat_kmat_ref.REF_DISCREPANCY = 5.55e-8, so the device bound stays
    PHI_TOL = 5.55e-7.  (The stopping rule r'r <= tol is absolute, so the rarest rows of the smallest N carry the
    largest scaled error: N = 61 on the dense K with 65 scanned rows reaches 5.71e-8, which is why the 65-row case
    of N = 61 is the CSR one and the dense one has as many entries as the case REF_DISCREPANCY was measured on.)

    pval.cond of the driver (golden rows, family K, conditioning on variants 30 and 77) from the float64 CG at
    tol = 1e-5 against the long-double Phi^K, relative: 4.96e-6 (binary, at most 4 steps a column), 1.6e-14
    (quantitative: tau[1] = 0 in the golden model): DRIVER_DISCREPANCY below is the larger, and the device's driver is
    held to 10 x that.
"""
import contextlib

import numpy as np

import skat_kmat_ref as M

TOL_SOLVE, MAXITER = M.TOL_SOLVE, M.MAXITER
# measured by tests/test_cond_kmat_ref.py::test_driver_pval_of_the_f64_reference_against_long_double (driver_case of
# tests/test_cond.py, K = family_K(1000), condition = [30, 77], mac = 4, tol = 1e-5)
DRIVER_DISCREPANCY = 4.96e-6
DRIVER_TOL = 10 * DRIVER_DISCREPANCY

# (name, N, covariates, trait, storage of K, n_cond, scanned rows, tau)
# N: lda padding / one slab, no multiple of 16 / two slabs of 2048 plus 3;  n_cond + K: one panel tile (<= 16) and two;
# rows: the edges of the 64-column chunk
CASES = [
    ("n61_k1_c1_csr", 61, 1, "binary", "csr", 1, 65, (1.0, 0.5)),
    ("n61_k3_c16_dense", 61, 3, "quantitative", "dense", 16, 1, (0.8, 0.4)),
    ("n1003_k3_c7_csr", 1003, 3, "binary", "csr", 7, 130, (1.0, 0.5)),
    ("n1003_k5_c16_dense", 1003, 5, "binary", "dense", 16, 64, (1.0, 0.3)),
    ("n4099_k5_c7_csr", 4099, 5, "quantitative", "csr", 7, 63, (0.9, 0.5)),
    ("n4099_k1_c1_csr", 4099, 1, "binary", "csr", 1, 65, (1.0, 0.8)),
]
_cases, _refs = {}, {}


def make_case(name):
    """A case of skat_kmat_ref.make_case's layout: rows 0 .. C-1 of ``packed`` are the set, the others are scanned."""
    if name in _cases:
        return _cases[name]
    from saigegds_amd.gds import pack_dosage_2bit
    import skat_ref as R
    _, n, kcov, trait, storage, n_cond, rows, tau = next(c for c in CASES if c[0] == name)
    mod, sm = M.flat_model(n, kcov, trait)
    codes = M.hard_calls(n, n_cond + rows, 97 + n + kcov + n_cond)
    if n_cond > 1 and rows > 1:        # the monomorphic row of hard_calls goes among the scanned rows where there are several
        codes[[1, n_cond]] = codes[[n_cond, 1]]
    K, csr, blocks = M.family_K(n) if storage == "csr" else (M.dense_K(n, 5 + n), None, None)
    c = dict(name=name, n=n, kcov=kcov, trait=trait, storage=storage, sm=sm, mod=mod, codes=codes, n_cond=n_cond,
             rows=rows, packed=pack_dosage_2bit(codes), lut=R.tables(codes), K=K, csr=csr, blocks=blocks,
             var_idx=np.arange(n_cond + rows, dtype=np.int32),
             w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.array(tau, dtype=np.float64))
    _cases[name] = c
    return c


def phi_rows(sm, packed, lut, n_cond, K, w, tau, form, blocks=None, tol=TOL_SOLVE, maxiter=MAXITER):
    """Rows 0 .. C-1 of ``packed`` the set, the others scanned -> dict(S [rows], var, cov [rows, C], S_C, Phi_CC, iters
    [C + rows] or None, units: per scanned row the [C + 1, C + 1] matrix Phi^K of (c_1 .. c_C, j))."""
    dtype = np.float64 if form == "f64" else np.longdouble
    tau = np.asarray(tau, dtype=np.float64)
    A, S = M.adj_columns(sm, packed, np.arange(packed.shape[0]), lut, dtype)
    X = np.asarray(sm.t_X, dtype=dtype).T
    if form == "f64":
        Z, _ = M.pcg_f64(K, w, tau, X, maxiter, tol)
        Y, iters = M.pcg_f64(K, w, tau, A, maxiter, tol)
    else:
        Z, Y, iters = M.solve_ld(K, w, tau, X, blocks), M.solve_ld(K, w, tau, A, blocks), None
    C = n_cond
    units = []
    for j in range(C, packed.shape[0]):
        idx = list(range(C)) + [j]
        units.append(M._phi(A[idx], X, Y[idx], Z, dtype))
    phi_cc = M._phi(A[:C], X, Y[:C], Z, dtype)
    return dict(S=S[C:], S_C=S[:C], Phi_CC=phi_cc, iters=iters, units=units,
                var=np.array([u[C, C] for u in units], dtype=dtype).reshape(-1),
                cov=np.array([u[C, :C] for u in units], dtype=dtype).reshape(-1, C))


def case_ref(name, form, tol=TOL_SOLVE):
    key = (name, form, tol)
    if key not in _refs:
        c = make_case(name)
        _refs[key] = phi_rows(c["sm"], c["packed"], c["lut"], c["n_cond"], c["K"], c["w"], c["tau"], form, c["blocks"], tol)
    return _refs[key]


def unit_matrix(phi_cc, cov_j, var_j):
    """[Phi_CC, Phi_Cj; Phi_jC, Phi_jj] of one scanned row."""
    C = phi_cc.shape[0]
    u = np.empty((C + 1, C + 1), dtype=np.result_type(phi_cc, cov_j))
    u[:C, :C], u[C, :C], u[:C, C], u[C, C] = phi_cc, cov_j, cov_j, var_j
    return u


def recording(Base):
    """``Base`` (the stand-in below or the real ``Scanner``) keeping what ``scan_2bit``, ``cond_kmat_set`` and
    ``cond_kmat`` returned; ``calls`` counts the scanners made, ``last`` is the most recent one."""
    class Rec(Base):
        calls = 0
        last = None

        def __init__(self, sm):
            Base.__init__(self, sm)
            Rec.calls += 1
            Rec.last = self
            self.scans, self.sets, self.rows = [], [], []

        def scan_2bit(self, packed):
            r = Base.scan_2bit(self, packed)
            self.scans.append(r)
            return r

        def cond_kmat_set(self, *a, **kw):
            r = Base.cond_kmat_set(self, *a, **kw)
            self.sets.append(r)
            return r

        def cond_kmat(self, *a, **kw):
            r = Base.cond_kmat(self, *a, **kw)
            self.rows.append(r)
            return r
    return Rec


def driver_inputs(rec):
    """What a recorded driver call fed ``cond_tests``: (kept rows x, scan table, S, var, cov, iters of all rows; the set's
    scan table, S_C, Phi_CC)."""
    out8 = np.concatenate([o for o, _ in rec.scans[1:]])
    valid = np.concatenate([v for _, v in rec.scans[1:]])
    S, var, cov, it = (np.concatenate([r[k] for r in rec.rows]) for k in range(4))
    return valid != 0, out8, S, var, cov, it, rec.scans[0][0], rec.sets[0][0], rec.sets[0][1]


def driver_expected(rec, binary, spa_pval=0.05, var=None, cov=None, Phi_CC=None):
    """``cond_tests`` on a recorded call's own outputs (or with ``var``, ``cov``, ``Phi_CC`` of all rows replaced) ->
    (kept rows, beta.cond, SE.cond, pval.cond, n.iter)."""
    from saigegds_amd.cond import cond_tests
    from saigegds_amd.skat import spa_scale
    x, out8, S, var0, cov0, it, out_c, S_C, phi0 = driver_inputs(rec)
    var, cov, Phi_CC = (var0 if var is None else var), (cov0 if cov is None else cov), (phi0 if Phi_CC is None else Phi_CC)
    d = d_C = None
    if binary:
        d = spa_scale(out8[x], S[x], var[x], spa_pval)
        d_C = spa_scale(out_c, S_C, np.diag(Phi_CC), spa_pval)
    beta, se, p = cond_tests(S[x], var[x], cov[x], S_C, Phi_CC, d, d_C)
    return x, np.where(out8[x, 0] > 0.5, -beta, beta), se, p, it[x]


def ref_cond_kmat_scanner_factory(form="f64", blocks=None):
    """The stand-in scanner of tests/test_cond.py with ``grm_operator``, ``cond_kmat_set`` and ``cond_kmat`` in one of the
    two reference forms (``blocks``: index ranges the matrix is block diagonal over, for the long-double solve), wrapped
    in ``recording``."""
    from test_cond import ref_cond_scanner_factory
    Base = ref_cond_scanner_factory()

    class RefCondKmatScanner(Base):
        @contextlib.contextmanager
        def grm_operator(self, mat):
            from saigegds_amd.grm import SparseGRM
            yield np.asarray(mat.to_dense() if isinstance(mat, SparseGRM) else mat, dtype=np.float64)

        def cond_kmat_set(self, op, packed_c, lut_c, w, tau, maxiter=500, tol=1e-5):
            self._kset = (np.array(packed_c), np.array(lut_c), np.asarray(w), np.asarray(tau), maxiter, tol)
            r = phi_rows(self._sm, self._kset[0], self._kset[1], packed_c.shape[0], op, w, tau, form, blocks, tol, maxiter)
            f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
            it = np.zeros(packed_c.shape[0], dtype=np.int32) if r["iters"] is None else r["iters"]
            return f(r["S_C"]), f(r["Phi_CC"]), it

        def cond_kmat(self, op, packed, lut):
            pc, lc, w, tau, maxiter, tol = self._kset
            C, m = pc.shape[0], packed.shape[0]
            ok = np.isfinite(lut).all(axis=1)
            S, var, cov, it = np.full(m, np.nan), np.full(m, np.nan), np.full((m, C), np.nan), np.zeros(m, dtype=np.int32)
            if ok.any():
                r = phi_rows(self._sm, np.concatenate([pc, packed[ok]]), np.concatenate([lc, lut[ok]]), C, op, w, tau,
                             form, blocks, tol, maxiter)
                S[ok], var[ok], cov[ok] = r["S"], r["var"], r["cov"]
                if r["iters"] is not None:
                    it[ok] = r["iters"][C:]
            return S, var, cov, it
    return recording(RefCondKmatScanner)
