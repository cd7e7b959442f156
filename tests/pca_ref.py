"""Reference of seqFitPCA for the CPU and GPU tests: structured genotypes, the long-double K of
grm_dense_ref.py, a numpy restatement of the block subspace iteration on a dense K, and the numpy stand-in operator the
driver's CPU tests inject.  No test functions here."""
import functools

import numpy as np

import grm_dense_ref as D
import grm_ref as R

from saigegds_amd.pca import PcaRankError

LD = np.longdouble
U = 2.0 ** -53

# (N, M, P): P populations, so P - 1 eigenvalues stand clear of the bulk; n_pc = P - 1, 1 % missing.  N just past a
# 256-sample tile, between tiles, and just past 1024 = the slab of the block Gram kernel.
DRIVER_CASES = [(257, 2000, 3), (600, 3000, 4), (1025, 1500, 3)]
MISS = 0.01
FST = 0.1
TOL, MAX_ITER, N_EXTRA = 1e-6, 100, 12
# the marker filter of the driver calls: every generated marker passes (ancestral frequency in 0.1 .. 0.9, 1 % missing)
FILTER = dict(maf=0.005, missing_rate=0.1)


def case_id(c):
    return "n%d-m%d-p%d" % c


@functools.lru_cache(maxsize=None)
def structured_codes(n, m, p, seed=5, miss=MISS):
    """[m, n] uint8 codes (3 = missing): Balding-Nichols populations of equal size around ancestral frequencies
    U(0.1, 0.9) with F_ST = FST, samples in population order, each entry missing at rate ``miss``.  Read-only."""
    rng = np.random.default_rng([seed, n, m, p])
    anc = rng.uniform(0.1, 0.9, m)
    a = (1 - FST) / FST
    freq = rng.beta(anc[:, None] * a, (1 - anc[:, None]) * a, size=(m, p))
    pop = (np.arange(n) * p) // n
    codes = rng.binomial(2, freq[:, pop]).astype(np.uint8)
    codes[rng.random((m, n)) < miss] = 3
    codes.setflags(write=False)
    return codes


def source(codes, prefix="s"):
    """An in-memory GenotypeSource of 2-bit rows."""
    from saigegds_amd.assoc import GenotypeSource
    n = codes.shape[1]
    return GenotypeSource([f"{prefix}{i}" for i in range(n)], packed=R.pack(codes))


@functools.lru_cache(maxsize=None)
def dense_K(n, m, p):
    """The long-double K of a driver case, and its eigenvalues (descending, of K rounded to double).  Read-only."""
    K = D.reference(structured_codes(n, m, p)).K
    lam = np.linalg.eigvalsh(K.astype(np.float64))[::-1].copy()
    K.setflags(write=False)
    lam.setflags(write=False)
    return K, lam


def sign_fix(vec):
    """Rows of vec with their entry of largest magnitude positive (the lowest index on ties) -> (vec, signs)."""
    vec = np.array(vec, dtype=np.float64)
    k = np.argmax(np.abs(vec), axis=1)
    s = np.where(vec[np.arange(vec.shape[0]), k] < 0, -1.0, 1.0)
    return vec * s[:, None], s


def _chol_qr(Q):
    """Columns of Q ([N, L]) -> Q R^-1, or PcaRankError at a pivot <= L 2^-52 max diag."""
    C = Q.T @ Q
    L = C.shape[0]
    thr = L * 2.0 ** -52 * np.max(np.diag(C))
    Rm = np.zeros_like(C)
    for j in range(L):
        for i in range(j + 1):
            s = C[i, j] - Rm[:i, i] @ Rm[:i, j]
            if i < j:
                Rm[i, j] = s / Rm[i, i]
            elif not s > thr:
                raise PcaRankError("the block lost rank")
            else:
                Rm[j, j] = np.sqrt(s)
    return np.linalg.solve(Rm.T, Q.T).T


def subspace_pca(K, n_pc, Q0, max_iter=MAX_ITER, tol=TOL):
    """The steps of sgx_grm_pca on a dense symmetric K in numpy double -> eigval, resid, vec [n_pc, N] (sign-fixed),
    signs, iters, n_converged."""
    K = np.asarray(K, dtype=np.float64)
    X = np.array(Q0, dtype=np.float64).T
    for it in range(1, int(max_iter) + 1):
        Q = _chol_qr(_chol_qr(X))
        Y = K @ Q
        H = Q.T @ Y
        th, V = np.linalg.eigh((H + H.T) / 2)
        th, V = th[::-1], V[:, ::-1]
        Um, W = Q @ V, Y @ V
        r = np.linalg.norm(W - Um * th[None, :], axis=0)
        ok = r[:n_pc] <= tol * th[0]
        if ok.all():
            break
        X = W
    vec, s = sign_fix(Um[:, :n_pc].T)
    lead = int(np.argmin(ok)) if not ok.all() else n_pc
    return {"eigval": th[:n_pc].copy(), "resid": r[:n_pc].copy(), "vec": vec, "signs": s, "iters": it, "n_converged": lead}


class NumpyPcaGrm(D.NumpyGrm):
    """grm_dense_ref.NumpyGrm with what seqFitPCA asks of an operator: pca(), marker_table()."""

    def _g(self):
        from saigegds_amd.gds import unpack_dosage_2bit
        codes = unpack_dosage_2bit(self.packed, self.n)
        af, inv = R.marker_stats(codes)
        return np.where(codes != 3, (codes.astype(np.float64) - 2 * af[:, None]) * inv[:, None], 0.0), af, inv

    def marker_table(self):
        return self._g()[1:]

    def marker_dots(self, B):
        return (self._g()[0] @ np.asarray(B, dtype=np.float64).T).T

    def pca(self, n_pc, Q0, max_iter=MAX_ITER, tol=TOL, loadings=False):
        r = subspace_pca(self.K, n_pc, Q0, max_iter, tol)
        r["loading"] = None
        if loadings:
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = np.where(r["eigval"] > 0, 1 / np.sqrt(self.m * r["eigval"]), 0.0)
            r["loading"] = self.marker_dots(r["vec"]) * sc[:, None]
        return r


def sine(u, v):
    """Sine of the angle between two vectors, without the cancellation of 1 - cos^2."""
    u, v = np.asarray(u, dtype=LD), np.asarray(v, dtype=LD)
    u, v = u / np.sqrt(u @ u), v / np.sqrt(v @ v)
    d = u - v * (v @ u)
    return float(np.sqrt(d @ d))
