"""Reference of the explicit-matrix operator (sgx_kmat, ``ExplicitGrmOperator``): long-double products, the numpy
stand-in with the operator interface, and builders of test matrices.  No test functions here.

Bound of a product: a double sum of nnz_i terms in any order, each an fma, is within
(nnz_i + 2) 2^-53 sum_j |K_ij| |b_j| of the exact sum (the first-order term is (nnz_i - 1) u; the margin of 3 u covers
the higher orders and the long-double reference's own rounding at these sizes).  Dense rows use n for nnz_i.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def full_pattern(n, i, j, x):
    """Upper triangle (i <= j) -> (rows, cols, vals) of both triangles, sorted by (row, col)."""
    i, j, x = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(x, dtype=np.float64)
    off = i != j
    r, c, v = np.concatenate([i, j[off]]), np.concatenate([j, i[off]]), np.concatenate([x, x[off]])
    o = np.lexsort((c, r))
    return r[o], c[o], v[o]


def csr_of(n, rows, cols, vals):
    """Sorted (rows, cols, vals) -> (row_ptr int64, col int32, val float64)."""
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(rows, dtype=np.int64), minlength=n), out=rp[1:])
    return rp, np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float64)


def csr_product_ld(n, rp, col, val, B):
    """-> (K B [k, n] long double, amplification sum_j |K_ij| |b_j| [k, n] long double, nnz per row)."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    rows = np.repeat(np.arange(n), np.diff(rp))
    out = np.zeros((B.shape[0], n), dtype=LD)
    amp = np.zeros((B.shape[0], n), dtype=LD)
    for k in range(B.shape[0]):
        t = val.astype(LD) * B[k][col].astype(LD)
        np.add.at(out[k], rows, t)
        np.add.at(amp[k], rows, np.abs(t))
    return out, amp, np.diff(rp)


def dense_product_ld(K, B):
    """-> (K B [k, n], amplification [k, n]) in long double, K [n, n], B [k, n]."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    Kl = np.asarray(K, dtype=np.float64).astype(LD)
    return (Kl @ B.astype(LD).T).T, (np.abs(Kl) @ np.abs(B).astype(LD).T).T


def assert_within_bound(got, ref, amp, nterms, what=""):
    """|got - ref| <= (nterms + 2) 2^-53 amp, element by element (nterms: [n] or a number)."""
    got = np.atleast_2d(np.asarray(got))
    bound = (np.asarray(nterms, dtype=LD) + 2) * LD(U) * amp
    err = np.abs(got.astype(LD) - ref)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float(np.max(err[bad] / np.maximum(bound[bad], LD(1e-300)))))


class KmatRef:
    """Numpy stand-in of the operator on an explicit matrix: a ``SparseGRM``-like object (i, j, x, n) or a square
    array.  Its PCG is PCG_diag_sigma's recurrence in double, so it serves as ``operator_factory`` of the fit."""

    def __init__(self, grm, n_samp=None):
        if hasattr(grm, "i") and hasattr(grm, "x"):
            self.n = int(grm.n)
            self.K = np.zeros((self.n, self.n))
            self.K[grm.i, grm.j] = grm.x
            self.K[grm.j, grm.i] = grm.x
        else:
            self.K = np.array(grm, dtype=np.float64)
            self.n = self.K.shape[0]
            if self.K.ndim != 2 or self.K.shape[1] != self.n:
                raise ValueError("the GRM must be a square matrix")
        assert n_samp is None or n_samp == self.n

    def diag(self):
        return np.diag(self.K).copy()

    def crossprod(self, b):
        return self.K @ np.asarray(b, dtype=np.float64)

    def crossprod_many(self, B):
        return np.stack([self.crossprod(b) for b in np.asarray(B)])

    def pcg(self, w, tau, b, maxiter=500, tol=1e-5):
        w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
        tau0, tau1 = float(tau[0]), float(tau[1])
        minv = 1.0 / np.maximum(tau0 / w + tau1 * np.diag(self.K), 1e-4)

        def sigma(p):
            base = tau0 * (p * (1 / w))
            return base + tau1 * (self.K @ p) if tau1 != 0 else base

        x = np.zeros(self.n)
        r = b.copy()
        z = minv * r
        p = z.copy()
        rr, rz = float(r @ r), float(r @ z)
        it = 0
        while it < maxiter and rr > tol:
            it += 1
            Ap = sigma(p)
            a = rz / float(p @ Ap)
            x = x + a * p
            r = r - a * Ap
            z = minv * r
            rz1 = float(z @ r)
            p = z + (rz1 / rz) * p
            rz, rr = rz1, float(r @ r)
        return x, it

    def pcg_many(self, w, tau, B, maxiter=500, tol=1e-5):
        res = [self.pcg(w, tau, b, maxiter, tol) for b in np.asarray(B)]
        return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)

    def matvec_ms(self):
        return 0.0

    def close(self):
        pass


def family_matrix(n, seed, big=0):
    """Upper triangle (i, j, x) of a PSD block-diagonal matrix on n samples: families of size 1..5, members
    consecutive, kinship 0.25 or 0.5 (one value per family) off the diagonal and a diagonal in [1.0, 1.1]; with
    ``big`` > 0 the first ``big`` samples form one block of kinship 0.25.  A block k J + (d_i - k) on the diagonal
    with 0 < k < d_i is positive definite."""
    rng = np.random.default_rng([seed, n, big])
    i, j, x = [], [], []
    s = 0
    first = True
    while s < n:
        if first and big:
            size, kin = min(big, n), 0.25
        else:
            size, kin = min(int(rng.integers(1, 6)), n - s), float(rng.choice([0.25, 0.5]))
        first = False
        d = rng.uniform(1.0, 1.1, size)
        for a in range(size):
            for b in range(a, size):
                i.append(s + a); j.append(s + b); x.append(d[a] if a == b else kin)
        s += size
    return np.array(i, dtype=np.int32), np.array(j, dtype=np.int32), np.array(x, dtype=np.float64)


class Upper:
    """The fields of a ``SparseGRM`` the operators read."""

    def __init__(self, n, i, j, x):
        self.n, self.i, self.j, self.x = int(n), np.asarray(i), np.asarray(j), np.asarray(x)

    def to_dense(self):
        K = np.zeros((self.n, self.n))
        K[self.i, self.j] = self.x
        K[self.j, self.i] = self.x
        return K
