"""References of the SKAT-O tests, written down plainly and apart from saigegds_amd/skato.py: the matrices ``B_rho`` by
way of an eigendecomposition of ``R``, the thresholds ``q_rho`` by bisection, and the Monte Carlo count of the event
``min_rho p_rho(s*) <= T`` under ``s* ~ N(0, A)``."""
import math

import numpy as np

RHO = (0, 0.01, 0.04, 0.09, 0.25, 0.5, 1)
N_DRAWS = 400_000
_cache = {}


def capped(rho):
    rho = np.asarray(rho, dtype=np.float64)
    return np.minimum(rho, 0.999) if rho.size > 1 else rho


def b_rho_plain(A, rho):
    """R^(1/2) A R^(1/2) with R = (1 - rho) I + rho 11', the square root from R's eigendecomposition."""
    m = A.shape[0]
    R = (1 - rho) * np.eye(m) + rho * np.ones((m, m))
    e, V = np.linalg.eigh(R)
    Rh = (V * np.sqrt(np.clip(e, 0, None))) @ V.T
    return Rh @ A @ Rh


def threshold(T, lam):
    """q with pchisq_mix(q, lam) = T: bisection in log q (pchisq_mix is non-increasing in q)."""
    from saigegds_amd.skat import pchisq_mix
    lo, hi = math.log(1e-12 * float(np.sum(lam))), math.log(float(np.sum(lam)))
    while pchisq_mix(math.exp(hi), lam) > T:
        hi += 1.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if pchisq_mix(math.exp(mid), lam) > T:
            lo = mid
        else:
            hi = mid
    return math.exp(0.5 * (lo + hi))


def block_case(m, n_block, seed, corr=0.5):
    """A covariance of m score statistics: correlation ``corr`` inside the first n_block, none elsewhere; seed = 0 gives
    unit variances, another seed variances within [0.5, 2]."""
    C = np.eye(m)
    C[:n_block, :n_block] = corr
    np.fill_diagonal(C, 1.0)
    if seed == 0:
        return C
    d = np.sqrt(np.random.default_rng(seed).uniform(0.5, 2.0, m))
    return C * d[:, None] * d[None, :]


def draws(A, seed=20240229):
    """N_DRAWS vectors s* ~ N(0, A) -> (sum s*^2, (sum s*)^2); made once per matrix and kept."""
    key = (A.tobytes(), seed)
    if key not in _cache:
        z = np.random.default_rng(seed).standard_normal((N_DRAWS, A.shape[0]))
        s = z @ np.linalg.cholesky(A).T
        _cache[key] = (np.sum(s * s, axis=1), np.sum(s, axis=1) ** 2)
    return _cache[key]


def monte_carlo(A, T, rho=RHO):
    """P(min_rho p_rho(s*) <= T) by counting draws with Q_rho(s*) >= q_rho for some rho -> (estimate, standard error)."""
    re = capped(rho)
    q0, q1 = draws(A)
    hit = np.zeros(q0.size, dtype=bool)
    for rk in re:
        lam = np.linalg.eigvalsh(b_rho_plain(A, rk))
        hit |= (1 - rk) * q0 + rk * q1 >= threshold(T, lam)
    p = float(hit.mean())
    return p, math.sqrt(p * (1 - p) / q0.size)
