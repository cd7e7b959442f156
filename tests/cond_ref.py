"""Reference of the conditional scan (sgx_cond_set / sgx_cond_2bit, saigegds_amd.cond) -- TEST INFRASTRUCTURE ONLY.

The dense adjusted genotypes of tests/skat_ref.py, adj = G - XXVX_inv (XV G), in ``np.longdouble`` by default:
    S_j = sum_i (y - mu)_i adj_ji,   Phi_jl = r sum_i mu2_i adj_ji adj_li        (quantitative: mu2 = 1, S / tau[0])
for the scanned rows against themselves (the diagonal only) and against the conditioning set, and the conditional test
formed directly: the score and the variance of the residual row adj_j - b adj_C, b the weighted least-squares
coefficients of adj_j on adj_C.  That shares nothing with cond_tests, which works on S and Phi alone.
"""
import numpy as np

import skat_ref as R


def solve(a, b):
    """a x = b by Gaussian elimination with partial pivoting in a's type (numpy.linalg has no long double)."""
    a, b = np.array(a), np.array(b)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]], b[[k, p]] = a[[p, k]], b[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:] -= f[:, None] * a[k][None, :]
        b[k + 1:] -= f[:, None] * b[k][None, :] if b.ndim == 2 else f * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - (a[k, k + 1:] @ x[k + 1:] if k + 1 < n else 0)) / a[k, k]
    return x


def cond_ref(sm, packed, lut, packed_c, lut_c, dtype=np.longdouble):
    """-> dict: S [m], var = Phi_jj [m], cov = Phi_jC [m, C], S_C [C], Phi_CC [C, C], T [m], V [m], all in ``dtype``."""
    m, c = np.asarray(packed).shape[0], np.asarray(packed_c).shape[0]
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)
    mu2 = np.ones(sm.n, dtype=dtype) if sm.quant else np.asarray(sm.mu2, dtype=dtype)
    y_mu = np.asarray(sm.y_mu, dtype=dtype)
    if sm.quant:
        y_mu = y_mu / dtype(sm.tau[0])
    r = dtype(sm.var_ratio)

    def adj_of(pk, lt, k):
        G = R.dosage_rows(pk, sm.n, np.arange(k), lt, dtype)
        return G - (G @ XV) @ XXVXi.T
    aC = adj_of(packed_c, lut_c, c)
    wC = aC * mu2
    out = dict(S_C=aC @ y_mu, Phi_CC=r * (wC @ aC.T))
    S, var, T, V = (np.zeros(m, dtype=dtype) for _ in range(4))
    cov = np.zeros((m, c), dtype=dtype)
    gram = wC @ aC.T
    for j0 in range(0, m, 64):                  # (in pieces: a long-double row of N = 70 001 is 1.1 MB)
        a = adj_of(np.asarray(packed)[j0:j0 + 64], np.asarray(lut).reshape(-1, 4)[j0:j0 + 64], min(64, m - j0))
        s = slice(j0, j0 + a.shape[0])
        S[s], var[s], cov[s] = a @ y_mu, r * np.sum(a * a * mu2, axis=1), r * (a @ wC.T)
        b = solve(gram, wC @ a.T).T             # [rows, C]
        res = a - b @ aC
        T[s], V[s] = res @ y_mu, r * np.sum(res * res * mu2, axis=1)
    out.update(S=S, var=var, cov=cov, T=T, V=V)
    return out
