"""SKAT-O, the optimal combination of burden and SKAT over a grid of correlations ``rho``, on MI355X:
``seqAssocGLMM_spaSKATO``, the combination ``skato_pvalue`` and the vectorised mixture tail ``pchisq_mix_vec``.

The reference has neither SKAT nor SKAT-O, so nothing here mirrors reference code and no reference vector pins it
(DESIGN.md 8k has the definition).  What ties it down: with a grid of one value it IS the SKAT driver's p-value
(``rho = 0``) or the burden chi-square (``rho = 1``); the device spectra are held against 40-digit eigenvalues; and the
combined p-value is held against a Monte Carlo count under ``s ~ N(0, A)`` (tests/test_skato.py, tests/test_gpu_skato.py).

The flow of a call is the SKAT driver's (skat.py) up to ``S`` and ``Phi`` per unit.  Then, per unit and weight column,
``s = w S`` and ``A = diag(w) Phi diag(w)``; the eigenvalues of the ``len(rho) + 1`` matrices ``B_rho`` and ``W`` of every
unit come from ONE ``sgx_skato_spectra`` call (a batched FP64 Jacobi kernel, kern_eig.h) while the scanner is still
open; units above ``SKATO_MAX_M`` variants, or a scanner without ``skato_spectra``, take ``np.linalg.eigvalsh``.  The
combination itself (root finding and a 128-point quadrature per unit) runs on the host.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import numpy as np

from .aggregate import AggrParamBeta, _dbeta, _run
from .skat import LAMBDA_DROP, LIMIT_T, _h_u, finish_skat, pchisq_mix, prepare_skat, unit_walk

RHO_DEFAULT = (0, 0.01, 0.04, 0.09, 0.25, 0.5, 1)
RHO_CAP = 0.999          # a grid of more than one value takes a value above this as this
X_MAX = 40.0             # the integral over the chi-square of the burden direction runs on (0, 40)
N_GL = 128               # Gauss-Legendre points of that integral, in z = sqrt(x)
_gl = {}


def check_rho(rho) -> np.ndarray:
    """The grid as a float64 vector: non-empty, within [0, 1], strictly increasing -- otherwise ``ValueError``."""
    try:
        g = np.asarray(rho, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("'rho' should be a numeric vector.") from None
    if g.size == 0 or not np.all(np.isfinite(g)) or g.min() < 0 or g.max() > 1:
        raise ValueError("'rho' should be a non-empty grid of values within [0, 1].")
    if np.any(np.diff(g) <= 0):
        raise ValueError("'rho' should be strictly increasing.")
    return g


def _rho_eff(rho: np.ndarray) -> np.ndarray:
    return np.minimum(rho, RHO_CAP) if rho.size > 1 else rho


def pchisq_mix_vec(q, lam) -> np.ndarray:
    """``pchisq_mix(q_i, lam)`` for a vector ``q`` and one ``lam``: the scalar function's steps (skat.pchisq_mix) on all
    ``q_i`` at once -- the same bracket, the same guarded Newton iteration per element (an element leaves the iteration
    where the scalar loop would break), the same closing formula.  Equal to the scalar function to rounding (1e-13
    relative is tested)."""
    from scipy.special import chdtrc, ndtr
    q = np.asarray(q, dtype=np.float64)
    shape = q.shape
    q = q.reshape(-1)
    lam = np.asarray(lam, dtype=np.float64).ravel()
    out = np.full(q.size, np.nan)
    if lam.size == 0 or not np.all(np.isfinite(lam)) or q.size == 0:
        return out.reshape(shape)
    lmax = float(lam.max())
    if not lmax > 0:
        return out.reshape(shape)
    fin = np.isfinite(q)
    out[fin & (q <= 0)] = 1.0
    pos = np.flatnonzero(fin & (q > 0))
    lam = lam[lam > LAMBDA_DROP * lmax]
    if lam.size == 1:
        out[pos] = chdtrc(1.0, q[pos] / lam[0])
        return out.reshape(shape)
    qq = q[pos]
    mean = float(lam.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(qq > mean, 0.0, np.where(qq < mean, -lam.size / (2 * qq), 0.0))
        hi = np.where(qq > mean, (1 - lmax / qq) / (2 * lmax), 0.0)
    t = np.zeros(qq.size)
    act = np.flatnonzero(lo < hi)
    l2 = lam * lam
    for _ in range(200):
        if act.size == 0:
            break
        ta = t[act]
        d = 1 - 2 * ta[:, None] * lam[None, :]
        f = (lam[None, :] / d).sum(axis=1) - qq[act]
        up = f > 0
        hi[act[up]] = ta[up]
        dn = f < 0
        lo[act[dn]] = ta[dn]
        k2 = 2 * (l2[None, :] / (d * d)).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tn = ta - f / k2
        la, ha = lo[act], hi[act]
        out_of = ~((la < tn) & (tn < ha))
        tn[out_of] = 0.5 * (la[out_of] + ha[out_of])
        zero = f == 0
        tn[zero] = ta[zero]                                  # (the scalar loop breaks before it moves)
        done = zero | (tn == ta) | (np.abs(tn - ta) <= 1e-16 * np.abs(tn))
        t[act] = tn
        act = act[~done]
    x = 2 * t[:, None] * lam[None, :]
    lim = np.abs(2 * t * lmax) < LIMIT_T
    res = np.empty(qq.size)
    if lim.any():
        k2 = 2 * float(l2.sum())
        res[lim] = float(ndtr(-(8 * float((l2 * lam).sum()) / (6 * k2 ** 1.5))))
    if (~lim).any():
        h, u = _h_u(x[~lim])
        sh = (l2[None, :] * h).sum(axis=1)
        w = 2 * t[~lim] * np.sqrt(sh)
        z = w + 0.5 * np.log1p((l2[None, :] * u).sum(axis=1) / (2 * sh)) / w
        res[~lim] = ndtr(-z)
    out[pos] = res
    return out.reshape(shape)


def skato_matrices(A, rho):
    """The ``len(rho) + 1`` symmetric matrices whose eigenvalues SKAT-O needs, as ``sgx_skato_spectra`` forms them:
    ``B_rho = R^(1/2) A R^(1/2)`` in closed form per grid value (a grid of more than one value takes a value above 0.999
    as 0.999), then ``W = A - r r' / c``.  ``rho = 0`` gives ``A`` itself, bit for bit."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    r = A.sum(axis=1)
    c = float(r.sum())
    mats = []
    for rk in _rho_eff(check_rho(rho)):
        a = math.sqrt(1 - rk)
        b = (math.sqrt(1 - rk + m * rk) - a) / m
        mats.append((a * a) * A + (a * b) * (r[:, None] + r[None, :]) + (b * b) * c)
    with np.errstate(divide="ignore", invalid="ignore"):
        mats.append(A - r[:, None] * (r[None, :] / c))
    return mats


def _gauss_legendre():
    if "z" not in _gl:
        x, w = np.polynomial.legendre.leggauss(N_GL)
        zmax = math.sqrt(X_MAX)
        _gl["z"], _gl["w"] = 0.5 * zmax * (x + 1), 0.5 * zmax * w
    return _gl["z"], _gl["w"]


def _quantile(T: float, q_from: float, lam: np.ndarray) -> float:
    """The root q >= q_from of pchisq_mix(q, lam) = T (pchisq_mix(q_from, lam) >= T), solved in log q by a bracketed
    method to 1e-13 relative."""
    from scipy.optimize import brentq
    f = lambda x: pchisq_mix(math.exp(x), lam) - T                         # noqa: E731
    lo = math.log(q_from)
    if not f(lo) > 0:
        return q_from
    hi = lo + 0.5
    while f(hi) > 0:
        hi += max(0.5, hi - lo)
        if hi > 700:
            return math.inf
    return math.exp(brentq(f, lo, hi, xtol=5e-14, rtol=8.9e-16, maxiter=200))


def skato_pvalue(s, A, rho=RHO_DEFAULT, spectra=None, _q0: Optional[float] = None) -> Dict[str, float]:
    """SKAT-O of one unit and weight column: ``s = w S`` the weighted score statistics, ``A = diag(w) Phi
    diag(w)`` their covariance, ``rho`` the grid -> ``{"pval", "p.SKAT", "p.burden", "T", "rho.min"}``.

    ``spectra``: None (the eigenvalues come from ``np.linalg.eigvalsh`` of ``skato_matrices(A, rho)``) or what
    ``Scanner.skato_spectra`` gives for this problem, ``[len(rho) + 1, m]``.  Per grid value ``Q_rho = (1 - rho) sum s^2 +
    rho (sum s)^2`` and ``p_rho = pchisq_mix(Q_rho, lam(rho))``; ``p.SKAT = p_0`` and ``p.burden = p_1 = chdtrc(1, (sum
    s)^2 / c)`` are given whether or not 0 and 1 are in the grid.  A grid of one value: ``pval = p_rho``.  Otherwise ``T =
    min p_rho`` at ``rho.min``, the thresholds ``q_rho`` with ``pchisq_mix(q_rho, lam(rho)) = T``, and ``pval = min(max(p_int,
    T), len(rho) T, 1)`` with ``p_int`` one minus the integral, over the chi-square ``x`` of the burden direction, of
    the mixture distribution function of the remainder ``W`` at ``delta(x)`` (128-point Gauss-Legendre in ``sqrt x``).
    No variant: NaN.  Non-finite ``A`` or ``s``: NaN.  ``c <= 0`` or one variant: ``pval = T = p.SKAT``, ``rho.min = 0``."""
    from scipy.special import chdtrc
    rho = check_rho(rho)
    s = np.asarray(s, dtype=np.float64).ravel()
    A = np.asarray(A, dtype=np.float64)
    m = s.size
    nan = float("nan")
    ans = {"pval": nan, "p.SKAT": nan, "p.burden": nan, "T": nan, "rho.min": nan}
    if m == 0 or A.shape != (m, m) or not np.all(np.isfinite(A)) or not np.all(np.isfinite(s)):
        return ans
    q0 = float(np.sum(s * s)) if _q0 is None else float(_q0)
    q1 = float(np.sum(s)) ** 2
    if not (math.isfinite(q0) and math.isfinite(q1)):
        return ans
    re = _rho_eff(rho)
    if spectra is None:
        spectra = [np.linalg.eigvalsh(B) if np.all(np.isfinite(B)) else np.full(m, nan) for B in skato_matrices(A, rho)]
    lam0 = spectra[0] if rho[0] == 0 else np.linalg.eigvalsh(A)
    r = A.sum(axis=1)
    c = float(r.sum())
    ans["p.SKAT"] = pchisq_mix(q0, lam0)
    if c > 0:
        ans["p.burden"] = float(chdtrc(1.0, q1 / c))
    if not c > 0 or m == 1:
        ans["pval"] = ans["T"] = ans["p.SKAT"]
        ans["rho.min"] = 0.0
        return ans
    Q = (1 - re) * q0 + re * q1
    p = np.array([ans["p.burden"] if rk == 1 else pchisq_mix(Q[k], spectra[k]) for k, rk in enumerate(re)])
    if not np.all(np.isfinite(p)):
        return ans
    kmin = int(np.argmin(p))
    T = float(p[kmin])
    ans["T"], ans["rho.min"] = T, float(rho[kmin])
    if rho.size == 1:
        ans["pval"] = T
        return ans
    if T <= 0 or T >= 1:
        ans["pval"] = T
        return ans
    qk = np.array([Q[k] if p[k] == T else _quantile(T, Q[k], np.asarray(spectra[k])) for k in range(rho.size)])
    lamW = np.clip(np.asarray(spectra[rho.size], dtype=np.float64), 0.0, None)
    rr = float(r @ r)
    tau = re * c + (1 - re) * rr / c
    muQ = float(lamW.sum())
    vz = 4 * (float(r @ A @ r) / c - rr * rr / (c * c))
    vQ = 2 * float(np.sum(lamW * lamW)) + vz
    if not np.all(np.isfinite(lamW)) or not math.isfinite(vQ):
        return ans
    if not (lamW.max() > 0 and vQ > 0 and vQ - vz > 0):
        # no remainder left (A of rank one): every Q_rho is tau(rho) times the one chi-square
        p_int = float(chdtrc(1.0, float(np.min(qk / tau))))
    else:
        z, wz = _gauss_legendre()
        x = z * z
        d = np.min((qk[None, :] - tau[None, :] * x[:, None]) / (1 - re)[None, :], axis=1)
        delta = (d - muQ) * math.sqrt((vQ - vz) / vQ) + muQ
        F = 1 - pchisq_mix_vec(delta, lamW)
        p_int = 1 - float(np.sum(wz * F * (2 * np.exp(-0.5 * x) / math.sqrt(2 * math.pi))))
    ans["pval"] = min(max(p_int, T), rho.size * T, 1.0)
    return ans


def seqAssocGLMM_spaSKATO(gdsfile, modobj, units, wbeta=AggrParamBeta, rho=RHO_DEFAULT, dsnode: str = "",
                          spa_pval: float = 0.05, var_ratio: float = float("nan"), res_savefn: str = "",
                          res_compress: str = "LZMA", parallel=False, verbose: bool = True, verbose_maf: bool = True,
                          scanner_factory=None, ds_budget: Optional[int] = None, grm_mat=None, tol_pcg: float = 1e-5,
                          maxiter_pcg: int = 500, collapse_mac: float = float("nan")) -> Dict[str, Any]:
    """SKAT-O per unit and weight set (not in the reference; arguments as ``seqAssocGLMM_spaSKAT`` plus the grid
    ``rho``: non-empty, within [0, 1], strictly increasing, else ``ValueError``).

    Everything up to ``S`` and ``Phi`` of a unit -- the scan at thresholds 0 / 0 / 1, the device Gram step on hard calls
    or on resident dosage batches, ``grm_mat=`` with ``Phi^K``, the SPA scaling of ``Phi`` on binary traits, the weights --
    is ``seqAssocGLMM_spaSKAT``'s own code with the same refusals (dosage input a scanner cannot serve, a LOCO model or
    more than one GPU with ``grm_mat``).  Then ``skato_pvalue`` per unit and weight column on ``s = w S`` and ``A = diag(w)
    Phi diag(w)``.  The eigenvalues of all units with at most ``SKATO_MAX_M`` variants come from one
    ``Scanner.skato_spectra`` call before the scanner is closed; larger units, and every unit where the scanner has no
    such method, take ``np.linalg.eigvalsh``.
    Columns: those of the burden driver's summary, ``n.var``, ``n.iter`` (only with ``grm_mat``), then ``pval``,
    ``pval.SKAT`` (``seqAssocGLMM_spaSKAT``'s ``pval``), ``pval.burden`` (the chi-square of ``(sum s)^2`` on one degree of
    freedom under the same covariance), ``rho.min`` and ``Q`` (SKAT's, ``sum w_j^2 S_j^2``), with the suffix ``.b<a>_<b>``
    where there is more than one weight set.  A unit with no variant left gives NaN.  ``collapse_mac``: as for
    ``seqAssocGLMM_spaSKAT`` (the same code; hard calls and dosage input alike), with its columns
    ``n.collapsed`` and ``mac.collapsed`` after ``n.var``."""
    from ._lib import SKATO_MAX_M
    rho = check_rho(rho)
    pr = prepare_skat("SAIGE SKAT-O analysis:", gdsfile, modobj, units, wbeta, dsnode, spa_pval, var_ratio, parallel, verbose,
                      scanner_factory, ds_budget, grm_mat, tol_pcg, maxiter_pcg, collapse_mac)
    try:
        _run(pr, skat=True)
        kept, n_iter, prob = [], [], []                     # prob: (unit, weight column, s, A, Q of SKAT)
        for u, r, S, phi, it in unit_walk(pr):
            kept.append(r)
            n_iter.append(it)
            if r.size == 0:
                continue
            for i, (wa, wb) in enumerate(pr.wbeta.T):
                w = _dbeta(pr.maf[r], wa, wb)
                prob.append((u, i, w * S, phi * w[:, None] * w[None, :], float(np.sum(w * w * S * S))))
        spectra = [None] * len(prob)
        dev = [j for j, p in enumerate(prob) if p[2].size <= SKATO_MAX_M and np.all(np.isfinite(p[3]))]
        if dev and hasattr(pr.sc, "skato_spectra"):
            lam, _ = pr.sc.skato_spectra([prob[j][3] for j in dev], rho)
            for j, x in zip(dev, lam):
                spectra[j] = x
    finally:
        pr.sc.close()
    nu, nw = len(kept), pr.wbeta.shape[1]
    cols = {c: np.full((nu, nw), np.nan) for c in ("pval", "pval.SKAT", "pval.burden", "rho.min", "Q")}
    for (u, i, s, A, q0), sp in zip(prob, spectra):
        res = skato_pvalue(s, A, rho, spectra=sp, _q0=q0)
        cols["Q"][u, i] = q0
        for c, key in (("pval", "pval"), ("pval.SKAT", "p.SKAT"), ("pval.burden", "p.burden"), ("rho.min", "rho.min")):
            cols[c][u, i] = res[key]
    return finish_skat(pr, kept, n_iter, cols, res_savefn, res_compress, verbose)
