"""Reference of sgx_ds_block_skat_kmat / sgx_ds_block_cond_kmat_set / sgx_ds_block_cond_kmat -- TEST
INFRASTRUCTURE ONLY.

Built on tests/skat_kmat_ref.py (models, K makers, the float64 CG with the device loop's stopping rule, the long-double
direct solve, ``_phi``, ``scaled_error``, the recorded bounds) and tests/skat_ds_ref.py (``dosage_G``: the dosage vector
of an entry exactly as it is defined).  Only the columns are new:

    G_e(i) = present(x) ? (flip[e] ? 2 - x : x) : mean[e],    adj_e = G_e - X (X'VX)^-1 X'V G_e

in float64 and in long double; an entry whose mean is not finite has a column of zeros and non-finite results.  The case
table of tests/test_gpu_kmat_ds.py and the numpy stand-in blocks of the driver tests are here too.

Recorded on the CPU (tests/test_kmat_ds_ref.py prints them), tol = 1e-12, maxiter = 500, scaled as
``skat_kmat_ref.scaled_error`` over the case table below (SKAT units, the set and every scanned row's unit):

    largest discrepancy of the float64 CG against long double   4.79e-8 (n61_k1_u8_csr; 5e-16 .. 5e-8 over the cases),
    RECORDED_REF below; it must stay within skat_kmat_ref.REF_DISCREPANCY = 5.55e-8, so the device bound stays
    PHI_TOL = 5.55e-7.  (The stopping rule r'r <= tol is absolute, so the rarest rows of N = 61 carry the largest scaled
    error, and it moves with the rows drawn -- 4.8e-8 .. 1.3e-7 over eight seeds of that case: the 65-row case is the
    one of N = 8195, and the seed of the rows is one that stays inside the project's bound.)

    pval of the drivers (fractional dosages, family K) from the float64 CG at tol = 1e-5 against the long-double
    Phi^K, relative: DRIVER_DISCREPANCY below; the device's drivers are held to 10 x that.
"""
import contextlib

import numpy as np

import skat_kmat_ref as M
import skat_ds_ref as SD
from aggregate_ds_ref import NA_INT
from cond_ds_ref import NumpyCondDsScanner, _NumpyCondDosageBlock

TOL_SOLVE, MAXITER = M.TOL_SOLVE, M.MAXITER
RECORDED_REF = 4.8e-8          # measured: 4.79e-8 (n61_k1_u8_csr); tests/test_kmat_ds_ref.py::test_f64_against_long_double
# measured by tests/test_kmat_ds_ref.py::test_driver_pvals_of_the_f64_reference_against_long_double: pval.cond 1.04e-5
# (fractional_case of tests/test_cond_dosage.py, condition = [30, 77], mac = 2), SKAT pval 7.71e-7 (100 rows of
# tests/test_skat_dosage.py's fractional_case in sliding windows of 12); K = family_K(1000), tol = 1e-5; the larger
DRIVER_DISCREPANCY = 1.04e-5
DRIVER_TOL = 10 * DRIVER_DISCREPANCY

# (name, N, covariates, trait, storage of K, block dtype, missing values, SKAT unit sizes, n_cond, scanned rows, tau)
# N: one partial 16-sample group / odd: rows that are aligned to their element only / two slabs of the products /
#    odd and two column-sum slabs of 8192 samples.  Covariates 16: seventeen sums a thread.  The rows of a case: the
#    first n_cond are the set, the others are scanned; the SKAT units run over all of them.  Row 1 holds equal values
#    (zeros), the last row of a case with missing values has every sample missing (its mean is not finite).
CASES = [
    ("n61_k1_u8_csr", 61, 1, "binary", "csr", np.uint8, True, (1, 16, 0, 17), 1, 33, (1.0, 0.5)),
    ("n61_k3_f64_dense", 61, 3, "quantitative", "dense", np.float64, False, (16, 1), 16, 1, (0.8, 0.4)),
    ("n1003_k16_f64_csr", 1003, 16, "binary", "csr", np.float64, True, (65, 0, 6), 7, 64, (1.0, 0.5)),
    ("n1003_k3_i32_dense", 1003, 3, "binary", "dense", np.int32, True, (17, 62), 16, 63, (1.0, 0.3)),
    ("n4099_k5_u8_csr", 4099, 5, "quantitative", "csr", np.uint8, False, (2, 6), 7, 1, (0.9, 0.5)),
    ("n8195_k3_f64_csr", 8195, 3, "binary", "csr", np.float64, True, (3, 0, 17, 46), 1, 65, (1.0, 0.8)),
]
_cases, _refs = {}, {}


def as_block_rows(codes, dtype, fractional_seed=None):
    """Hard calls (0, 1, 2, 3 = missing) as rows of a dosage block of ``dtype``; ``fractional_seed``: float64 rows
    become imputed-looking dosages in [0, 2] around the calls."""
    codes = np.asarray(codes).astype(np.int64)
    miss = codes == 3
    if np.dtype(dtype) == np.uint8:
        return np.where(miss, 0xFF, codes).astype(np.uint8)
    if np.dtype(dtype) == np.int32:
        return np.where(miss, NA_INT, codes).astype(np.int32)
    x = codes.astype(np.float64)
    if fractional_seed is not None:
        rng = np.random.default_rng(fractional_seed)
        x = np.clip(x + np.where(x > 0, rng.uniform(-0.45, 0.45, x.shape), rng.uniform(0, 0.05, x.shape) ** 2), 0, 2)
    return np.where(miss, np.nan, x)


def make_case(name):
    """The inputs of a case, made once: model, block rows, flip / mean of every row (the drivers' own), units, K, w, tau."""
    if name in _cases:
        return _cases[name]
    _, n, kcov, trait, storage, dtype, missing, units, n_cond, rows, tau = next(c for c in CASES if c[0] == name)
    mod, sm = M.flat_model(n, kcov, trait)
    m_tot = n_cond + rows
    assert int(sum(units)) == m_tot
    codes = M.hard_calls(n, m_tot, 60 + n + kcov + n_cond)
    if not missing:
        codes[codes == 3] = 0
    if n_cond > 1:                     # the row of equal values goes among the scanned rows
        codes[[1, n_cond]] = codes[[n_cond, 1]]
    zero_row = n_cond if n_cond > 1 else 1
    ds = as_block_rows(codes, dtype, fractional_seed=7 + n)
    if m_tot > 1:
        ds[zero_row] = as_block_rows(np.where(codes[zero_row] == 3, 3, 0), dtype)
    if missing:
        ds[-1] = as_block_rows(np.full(n, 3), dtype)
    flip, mean = SD.flip_mean(ds)
    K, csr, blocks = M.family_K(n) if storage == "csr" else (M.dense_K(n, 5 + n), None, None)
    c = dict(name=name, n=n, kcov=kcov, trait=trait, storage=storage, dtype=np.dtype(dtype), sm=sm, mod=mod, rows=ds,
             flip=flip, mean=mean, n_cond=n_cond, var_idx=np.arange(m_tot, dtype=np.int32),
             unit_ptr=np.concatenate([[0], np.cumsum(units)]).astype(np.int64), K=K, csr=csr, blocks=blocks,
             w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.array(tau, dtype=np.float64))
    _cases[name] = c
    return c


def adj_columns(sm, rows, var_idx, flip, mean, dtype):
    """A [entries, N]: adj_e = G_e - XXVX_inv (XV G_e) with G of ``skat_ds_ref.dosage_G``, the score statistics S_e
    (quantitative: / tau[0]) and the entries whose mean is not finite (a column of zeros; S is NaN there)."""
    mean = np.asarray(mean, dtype=np.float64)
    bad = ~np.isfinite(mean)
    G = SD.dosage_G(rows, var_idx, flip, np.where(bad, 0.0, mean), dtype)
    G[bad] = 0
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)
    A = G - (G @ XV) @ XXVXi.T
    S = A @ np.asarray(sm.y_mu, dtype=dtype)
    S = S / dtype(sm.tau[0]) if sm.quant else S
    S[bad] = np.nan
    return A, S, bad


def solved(sm, rows, var_idx, flip, mean, K, w, tau, form, blocks=None, tol=TOL_SOLVE, maxiter=MAXITER):
    """The columns of the entries and their solves in one of the two forms -> dict(A, S, bad, X, Y, Z, iters or None)."""
    dtype = np.float64 if form == "f64" else np.longdouble
    tau = np.asarray(tau, dtype=np.float64)
    A, S, bad = adj_columns(sm, rows, var_idx, flip, mean, dtype)
    X = np.asarray(sm.t_X, dtype=dtype).T
    if form == "f64":
        Z, _ = M.pcg_f64(K, w, tau, X, maxiter, tol)
        Y, iters = M.pcg_f64(K, w, tau, A, maxiter, tol)
    else:
        Z, Y, iters = M.solve_ld(K, w, tau, X, blocks), M.solve_ld(K, w, tau, A, blocks), None
    return dict(A=A, S=S, bad=bad, X=X, Y=Y, Z=Z, iters=iters, dtype=dtype)


def phi_of(s, idx):
    """Phi^K of the entries ``idx`` of ``solved``'s result as one unit; NaN in the rows and columns of its bad entries."""
    idx = np.asarray(idx, dtype=np.int64)
    p = M._phi(s["A"][idx], s["X"], s["Y"][idx], s["Z"], s["dtype"])
    b = s["bad"][idx]
    p[b, :] = np.nan
    p[:, b] = np.nan
    return p


def phi_units(c, form, tol=TOL_SOLVE, maxiter=MAXITER, tau=None):
    """SKAT: (score [entries], [Phi^K of unit u], iters or None) of a case."""
    s = solved(c["sm"], c["rows"], c["var_idx"], c["flip"], c["mean"], c["K"], c["w"], c["tau"] if tau is None else tau,
               form, c["blocks"], tol, maxiter)
    up = c["unit_ptr"]
    return s["S"], [phi_of(s, np.arange(up[u], up[u + 1])) for u in range(len(up) - 1)], s["iters"]


def phi_rows(sm, rows, flip, mean, n_cond, K, w, tau, form, blocks=None, tol=TOL_SOLVE, maxiter=MAXITER):
    """The conditional scan: rows 0 .. C-1 the set, the others scanned -> dict as ``cond_kmat_ref.phi_rows``."""
    s = solved(sm, rows, np.arange(len(rows)), flip, mean, K, w, tau, form, blocks, tol, maxiter)
    C, dtype = n_cond, s["dtype"]
    units = [phi_of(s, list(range(C)) + [j]) for j in range(C, len(rows))]
    return dict(S=s["S"][C:], S_C=s["S"][:C], Phi_CC=phi_of(s, np.arange(C)), iters=s["iters"], units=units,
                var=np.array([u[C, C] for u in units], dtype=dtype).reshape(-1),
                cov=np.array([u[C, :C] for u in units], dtype=dtype).reshape(-1, C))


def case_ref(name, form, tol=TOL_SOLVE, tau=None):
    """Both references of a case from one set of solves, made once: dict(S [all rows], iters, skat: [Phi^K of SKAT unit
    u], and the conditional scan's S_C, Phi_CC, units, var, cov as ``phi_rows`` gives them)."""
    key = (name, form, tol, None if tau is None else tuple(tau))
    if key not in _refs:
        c = make_case(name)
        s = solved(c["sm"], c["rows"], c["var_idx"], c["flip"], c["mean"], c["K"], c["w"], c["tau"] if tau is None else tau,
                   form, c["blocks"], tol)
        up, C, m = c["unit_ptr"], c["n_cond"], len(c["rows"])
        units = [phi_of(s, list(range(C)) + [j]) for j in range(C, m)]
        _refs[key] = dict(S=s["S"], iters=s["iters"], skat=[phi_of(s, np.arange(up[u], up[u + 1])) for u in range(len(up) - 1)],
                          S_C=s["S"][:C], Phi_CC=phi_of(s, np.arange(C)), units=units,
                          var=np.array([u[C, C] for u in units], dtype=s["dtype"]).reshape(-1),
                          cov=np.array([u[C, :C] for u in units], dtype=s["dtype"]).reshape(-1, C))
    return _refs[key]


def finite_error(cov, ref):
    """``skat_kmat_ref.scaled_error`` over the entries whose reference is finite; the non-finite patterns must agree."""
    cov, ref = np.asarray(cov), np.asarray(ref)
    nan = ~np.isfinite(np.asarray(ref, dtype=np.float64))
    assert np.array_equal(~np.isfinite(np.asarray(cov, dtype=np.float64)), nan), "non-finite patterns differ"
    keep = ~nan.all(axis=1)
    if not keep.any():
        return 0.0
    return M.scaled_error(cov[np.ix_(keep, keep)], ref[np.ix_(keep, keep)])


# ---- stand-ins of the driver tests ----------------------------------------------------------------------------------
class _NumpyKmatDosageBlock(_NumpyCondDosageBlock):
    """``_NumpyCondDosageBlock`` with ``skat_kmat``, ``cond_kmat_set`` and ``cond_kmat`` in one of the two reference forms
    (the scanner's ``kmat_form`` / ``kmat_blocks``); ``op`` is the dense matrix the scanner's ``grm_operator`` yields."""

    def _solved(self, rows, var_idx, flip, mean, op, w, tau, maxiter, tol):
        sc = self.sc
        return solved(sc._sm, rows, var_idx, flip, mean, op, w, tau, sc.kmat_form, sc.kmat_blocks, tol, maxiter)

    def skat_kmat(self, op, unit_ptr, var_idx, flip, mean, w, tau, maxiter=500, tol=1e-5):
        f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
        s = self._solved(self.rows, var_idx, flip, mean, op, w, tau, maxiter, tol)
        n = len(var_idx)
        it = np.zeros(n, dtype=np.int32) if s["iters"] is None else s["iters"]
        r = (f(s["S"]), [f(phi_of(s, np.arange(unit_ptr[u], unit_ptr[u + 1]))) for u in range(len(unit_ptr) - 1)], it)
        self.sc.kmat_log.append(("skat", r))
        return r

    def cond_kmat_set(self, op, var_idx, flip, mean, w, tau, maxiter=500, tol=1e-5):
        var_idx = np.asarray(var_idx, dtype=np.int64)
        self.sc._kset = (np.array(self.rows[var_idx]), np.array(flip), np.array(mean), np.asarray(w), np.asarray(tau),
                         maxiter, tol)
        s = self._solved(self.sc._kset[0], np.arange(var_idx.size), flip, mean, op, w, tau, maxiter, tol)
        f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
        it = np.zeros(var_idx.size, dtype=np.int32) if s["iters"] is None else s["iters"]
        r = (f(s["S"]), f(phi_of(s, np.arange(var_idx.size))), it)
        self.sc.kmat_log.append(("set", r))
        return r

    def cond_kmat(self, op, flip, mean):
        rc, fc, mc, w, tau, maxiter, tol = self.sc._kset
        C, m = len(rc), len(self.rows)
        sc = self.sc
        r = phi_rows(sc._sm, np.concatenate([rc, self.rows]), np.concatenate([fc, flip]), np.concatenate([mc, mean]), C,
                     op, w, tau, sc.kmat_form, sc.kmat_blocks, tol, maxiter)
        f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
        it = np.zeros(m, dtype=np.int32) if r["iters"] is None else r["iters"][C:]
        out = (f(r["S"]), f(r["var"]), f(r["cov"]), it)
        self.sc.kmat_log.append(("rows", out))
        return out


def kmat_ds_scanner_factory(form="f64", blocks=None):
    """``NumpyCondDsScanner`` with ``grm_operator`` and a dosage block that has the three explicit-GRM methods;
    ``kmat_log`` keeps what they returned, ``scan_log`` what the blocks' scans returned, ``last`` the scanner made last."""
    from saigegds_amd.grm import SparseGRM

    class Block(_NumpyKmatDosageBlock):
        def scan(self):
            r = _NumpyKmatDosageBlock.scan(self)
            self.sc.scan_log.append(r)
            return r

    class KmatDsScanner(NumpyCondDsScanner):
        last = None
        kmat_form, kmat_blocks = form, blocks

        def __init__(self, sm):
            super().__init__(sm)
            self.kmat_log, self.scan_log, self._kset = [], [], None
            KmatDsScanner.last = self

        @contextlib.contextmanager
        def grm_operator(self, mat):
            yield np.asarray(mat.to_dense() if isinstance(mat, SparseGRM) else mat, dtype=np.float64)

        def dosage_block(self, dtype, max_variants):
            return Block(self, dtype, max_variants)
    return KmatDsScanner
