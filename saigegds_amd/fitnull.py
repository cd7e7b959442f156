"""Null-model fit: Python mirror of ``seqFitNullGLMM_SPA()``.

Host driver (reference R/saige_main.r:223-654) and the AI-REML / PCG loop of
src/saige_fitnull.cpp:739-1474, written around the implicit-GRM operator of
``libsaigehip.so`` (``sgx_grm_*``, reference :159-230, 435-536, 581-614).  All
heavy work -- every ``PCG_diag_sigma`` solve and every ``get_crossprod_b_grm``
product -- runs on the GPU; what stays here is K x K dense algebra, the glm
start values and the reference's control flow.

Random numbers.  The reference draws its Hutchinson trace vectors with R's
``rbinom`` after ``set.seed(seed)`` and picks the variance-ratio markers with
``sample.int``.  To reproduce a model bit-for-bit in its random choices the
generator is restated: Mersenne-Twister with R's seed scrambling, ``unif_rand``,
``rbinom(n, 1, 0.5)`` (inversion branch) and ``sample.int`` with
``sample.kind = "Rounding"`` (what the reference's test suite selects,
inst/unitTests/test_SAIGE.R:15,48).
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .gds import GdsFile, pack_dosage_2bit, unpack_dosage_2bit
from .nullmod import NullModel

# ---------------------------------------------------------------------------
# R's random number stream


class RRandom:
    """``RNGkind("Mersenne-Twister", "Inversion", "Rounding")``.

    The 32-bit generator is MT19937 itself (numpy's bit generator with the key
    words R's ``set.seed`` produces), so bulk draws are vectorised."""

    _I2_32M1 = 2.328306437080797e-10

    def __init__(self, seed: int = 0):
        self._bg = np.random.MT19937()
        self.set_seed(seed)

    def set_seed(self, seed: int):
        """``set.seed(seed)``: RNG_Init of R's RNG.c (initial scrambling, then
        625 LCG words: mti and the state; FixupSeeds sets mti = 624)."""
        s = int(seed) & 0xFFFFFFFF
        for _ in range(50):
            s = (69069 * s + 1) & 0xFFFFFFFF
        words = np.empty(625, dtype=np.uint32)
        for i in range(625):
            s = (69069 * s + 1) & 0xFFFFFFFF
            words[i] = s
        self._bg.state = {"bit_generator": "MT19937", "state": {"key": words[1:].copy(), "pos": 624}}

    def unif(self, n: int) -> np.ndarray:
        """``runif(n)``: MT_genrand * 2^-32, then fixup() into (0, 1)."""
        v = self._bg.random_raw(int(n)).astype(np.float64) * 2.3283064365386963e-10
        v[v <= 0.0] = 0.5 * self._I2_32M1
        v[1.0 - v <= 0.0] = 1.0 - 0.5 * self._I2_32M1
        return v

    def unif_rand(self) -> float:
        return float(self.unif(1)[0])

    def rbinom1_half(self, n: int) -> np.ndarray:
        """``rbinom(n, 1, 0.5)``: the inversion branch of rbinom.c reduces to
        ``unif_rand() >= 0.5``."""
        return (self.unif(n) >= 0.5).astype(np.float64)

    def sample_int(self, n: int) -> np.ndarray:
        """``sample.int(n, n)`` without replacement, sample.kind "Rounding"
        (do_sample -> R_unif_index = floor(dn * unif_rand()))."""
        js = np.floor(np.arange(n, 0, -1, dtype=np.float64) * self.unif(n)).astype(np.int64).tolist()
        x = list(range(1, n + 1))
        out = [0] * n
        nn = n
        for i, j in enumerate(js):
            out[i] = x[j]
            nn -= 1
            x[j] = x[nn]
        return np.asarray(out, dtype=np.int64)


# ---------------------------------------------------------------------------
# glm families and IRLS (stats::glm.fit)


class Family:
    def __init__(self, name: str):
        self.name = name

    def linkinv(self, eta):
        if self.name == "binomial":
            return 1.0 / (1.0 + np.exp(-eta))
        return eta

    def mu_eta(self, eta):
        if self.name == "binomial":
            e = np.exp(-np.abs(eta))
            return np.maximum(e / (1 + e) ** 2, np.finfo(float).eps)
        return np.ones_like(eta)

    def variance(self, mu):
        if self.name == "binomial":
            return mu * (1 - mu)
        return np.ones_like(mu)


@dataclass
class GlmFit:
    family: Family
    coefficients: np.ndarray
    linear_predictors: np.ndarray
    fitted_values: np.ndarray
    y: np.ndarray
    residuals: np.ndarray     # working residuals for gaussian = response residuals
    offset: Optional[np.ndarray] = None


def glm_fit(X: np.ndarray, y: np.ndarray, family: str) -> GlmFit:
    """``glm(formula, family)`` by IRLS to the defaults epsilon=1e-8, maxit=25."""
    fam = Family(family)
    if family == "gaussian":
        coef = np.linalg.lstsq(X, y, rcond=None)[0]
        eta = X @ coef
        return GlmFit(fam, coef, eta, eta.copy(), y.copy(), y - eta)
    mu = (y + 0.5) / 2.0
    eta = np.log(mu / (1 - mu))
    dev_old = np.inf
    coef = np.zeros(X.shape[1])
    for _ in range(25):
        me = fam.mu_eta(eta)
        z = eta + (y - mu) / me
        w = np.sqrt(me * me / fam.variance(mu))
        coef = np.linalg.lstsq(X * w[:, None], z * w, rcond=None)[0]
        eta = X @ coef
        mu = fam.linkinv(eta)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = 2 * (np.where(y > 0, y * np.log(y / mu), 0.0) + np.where(y < 1, (1 - y) * np.log((1 - y) / (1 - mu)), 0.0))
        dev = float(d.sum())
        if abs(dev - dev_old) / (abs(dev) + 0.1) < 1e-8:
            break
        dev_old = dev
    return GlmFit(fam, coef, eta, mu, y.copy(), (y - mu) / fam.mu_eta(eta))


# ---------------------------------------------------------------------------
# AI-REML pieces of src/saige_fitnull.cpp


def _mat_inv(m: np.ndarray) -> np.ndarray:
    """``mat_inv`` (:722-733): inverse of the symmetrised matrix."""
    xs = np.triu(m) + np.triu(m, 1).T
    try:
        c = np.linalg.cholesky(xs)
        ci = np.linalg.inv(c)
        return ci.T @ ci
    except np.linalg.LinAlgError:
        return np.linalg.inv(xs)


def _calc_cv(x: np.ndarray) -> float:
    """``calcCV`` (:618-623)."""
    return float(np.std(x, ddof=1) / (np.mean(x) * len(x)))


@dataclass
class _Param:
    seed: int
    tol: float
    tolPCG: float
    maxiter: int
    maxiterPCG: int
    nrun: int
    num_marker: int
    traceCVcutoff: float
    ratioCVcutoff: float
    verbose: bool


class _Fitter:
    """The algorithm is written once, on ``solve`` and ``products``: rows of right-hand sides that share
    (w, tau) -- Y and the columns of X, the trace vectors, the columns of X1 -- in, rows out.  Only those
    two methods know how the rows reach the operator: ``batched`` and an operator with ``pcg_many`` /
    ``crossprod_many`` take them in one call, anything else one ``pcg`` / ``crossprod`` per row, in row
    order.  The operators give every row of a batched call the bits of its single call, so ``batched`` is a
    cost choice and changes no result."""

    def __init__(self, op, X: np.ndarray, y: np.ndarray, fit0: GlmFit, param: _Param, rng: RRandom,
                 batched: bool = False):
        self.op, self.X, self.y, self.fit0, self.p, self.rng = op, X, y, fit0, param, rng
        self.fam = fit0.family
        self.offset = np.zeros_like(y) if fit0.offset is None else fit0.offset
        self.batched = batched

    def pcg(self, w, tau, b):
        x, _ = self.op.pcg(w, tau, b, self.p.maxiterPCG, self.p.tolPCG)
        return x

    def solve(self, w, tau, B):
        """Solves of the rows of B ([k, N]) -> [k, N]."""
        if self.batched and hasattr(self.op, "pcg_many"):
            return self.op.pcg_many(w, tau, B, self.p.maxiterPCG, self.p.tolPCG)[0]
        return np.stack([self.pcg(w, tau, np.ascontiguousarray(b)) for b in B])

    def products(self, B):
        """GRM products of the rows of B ([k, N]) -> [k, N]."""
        if self.batched and hasattr(self.op, "crossprod_many"):
            return self.op.crossprod_many(B)
        return np.stack([self.op.crossprod(np.ascontiguousarray(b)) for b in B])

    # get_coeff_w (:739-758)
    def get_coeff_w(self, Y, w, tau, S=None):
        """``S``: the solves of Y and of the columns of X ([1 + K, N]) where the caller has them already."""
        X = self.X
        if S is None:
            S = self.solve(w, tau, np.vstack([Y[None, :], X.T]))
        Sigma_iY, Sigma_iX = S[0], np.ascontiguousarray(S[1:].T)
        cov = _mat_inv(X.T @ Sigma_iX)
        alpha = cov @ (Sigma_iX.T @ Y)
        eta = Y - tau[0] * (Sigma_iY - Sigma_iX @ alpha) / w
        return Sigma_iY, Sigma_iX, cov, alpha, eta

    def working(self, eta):
        """mu, the working response Y and the IRLS weights W at eta (offset included)."""
        fam, y, offset = self.fam, self.y, self.offset
        mu = fam.linkinv(eta)
        mu_eta = fam.mu_eta(eta)
        Y = eta - offset + (y - mu) / mu_eta
        W = mu_eta * mu_eta / fam.variance(mu)
        return mu, Y, W

    def irls_step(self, Y, W, tau, a0, S=None):
        """One step of get_coeff from the state (Y, W), ``S`` as for get_coeff_w -> (the next state: get_coeff's
        dict, whether alpha is within the criterion of a0)."""
        tol_coef = 0.1
        Sigma_iY, Sigma_iX, cov, alpha, eta = self.get_coeff_w(Y, W, tau, S)
        eta = eta + self.offset
        mu, Y, W = self.working(eta)
        done = np.max(np.abs(alpha - a0) / (np.abs(alpha) + np.abs(a0) + tol_coef)) < tol_coef
        return dict(Y=Y, mu=mu, alpha=alpha, eta=eta, W=W, cov=cov, Sigma_iY=Sigma_iY, Sigma_iX=Sigma_iX), done

    # get_coeff (:778-813)
    def get_coeff(self, tau, alpha0, eta0):
        mu, Y, W = self.working(eta0)
        a0 = alpha0
        for _ in range(self.p.maxiter):
            c, done = self.irls_step(Y, W, tau, a0)
            if done:
                break
            Y, W, a0 = c["Y"], c["W"], c["alpha"]
        return c

    def get_coeff_lockstep(self, tau, alpha0, eta0, keys, solve):
        """``get_coeff`` for several operators at once (the leave-one-chromosome-out models, SAIGE's
        Get_Coef_LOCO): every key starts from (alpha0, eta0) and takes get_coeff's IRLS steps with its own
        W, and leaves the step list when its own alpha criterion is met.  ``solve(act, B, W)`` solves, for
        every key in ``act``, the 1 + K right-hand sides ``B[key]`` ([1 + K, N]: Y, then the columns of X)
        with the weights ``W[key]`` on that key's operator -> {key: (S [1 + K, N], iters [1 + K])}.
        -> {key: get_coeff's dict plus steps (IRLS steps taken) and pcg_iters ([steps, 1 + K])}."""
        X = self.X
        st = {}
        for k in keys:
            mu, Y, W = self.working(eta0)
            st[k] = dict(Y=Y, mu=mu, W=W, a0=alpha0, steps=0, pcg_iters=[])
        act = list(keys)
        for _ in range(self.p.maxiter):
            if not act:
                break
            S = solve(act, {k: np.vstack([st[k]["Y"][None, :], X.T]) for k in act}, {k: st[k]["W"] for k in act})
            still = []
            for k in act:
                c = st[k]
                Sk, its = S[k]
                nxt, done = self.irls_step(c["Y"], c["W"], tau, c["a0"], Sk)
                c.update(nxt, steps=c["steps"] + 1)
                c["pcg_iters"].append([int(v) for v in its])
                if not done:
                    c["a0"] = nxt["alpha"]
                    still.append(k)
            act = still
        return st

    # get_trace (:627-668) / get_trace_q (:672-718)
    def get_trace(self, Sigma_iX, w, tau, cov, quant: bool):
        p, n = self.p, self.op.n
        self.rng.set_seed(p.seed)
        nrun_start, nrun_end = 0, p.nrun
        buf, buf0 = np.zeros(p.nrun), np.zeros(p.nrun)
        while True:
            # the round's vectors in the reference's draw order (only the draws consume the generator), then their
            # solves, then their products
            U = np.stack([2 * self.rng.rbinom1_half(n) - 1 for _ in range(nrun_start, nrun_end)])
            SU, AU = self.solve(w, tau, U), self.products(U)
            for i in range(nrun_start, nrun_end):
                u, Sigma_iu, Au = U[i - nrun_start], SU[i - nrun_start], AU[i - nrun_start]
                Pu = Sigma_iu - Sigma_iX @ (cov @ (Sigma_iX.T @ u))
                buf[i] = float(Au @ Pu)
                buf0[i] = float(u @ Pu)
            cv = _calc_cv(buf)
            cv0 = _calc_cv(buf0) if quant else 0.0
            if cv > p.traceCVcutoff or cv0 > p.traceCVcutoff:
                nrun_start, nrun_end = nrun_end, nrun_end + 10
                buf = np.concatenate([buf, np.zeros(10)])
                buf0 = np.concatenate([buf0, np.zeros(10)])
                if p.verbose:
                    print(f"CV for trace random estimator using {p.nrun} runs is {max(cv, cv0):g} > {p.traceCVcutoff:g}")
                    print(f"try {nrun_end} runs ...")
                continue
            break
        return (float(np.mean(buf0)), float(np.mean(buf))) if quant else float(np.mean(buf))

    def _proj(self, v, Sigma_iX, cov):
        return v - Sigma_iX @ (cov @ (Sigma_iX.T @ v))

    # get_AI_score (:817-833)
    def get_AI_score(self, Y, w, tau, Sigma_iY, Sigma_iX, cov):
        PY = Sigma_iY - Sigma_iX @ (cov @ (Sigma_iX.T @ Y))
        APY = self.op.crossprod(PY)
        YPAPY = float(PY @ APY)
        trace = self.get_trace(Sigma_iX, w, tau, cov, quant=False)
        PAPY_1 = self.pcg(w, tau, APY)
        PAPY = PAPY_1 - Sigma_iX @ (cov @ (Sigma_iX.T @ PAPY_1))
        return YPAPY, trace, float(APY @ PAPY)

    # get_AI_score_q (:836-864)
    def get_AI_score_q(self, Y, w, tau, Sigma_iY, Sigma_iX, cov):
        PY = Sigma_iY - Sigma_iX @ (cov @ (Sigma_iX.T @ Y))
        A0PY = PY
        APY = self.op.crossprod(PY)
        YPAPY = (float(PY @ APY), float(PY @ A0PY))
        trace = self.get_trace(Sigma_iX, w, tau, cov, quant=True)
        AI = np.zeros((2, 2))
        PA0PY_1 = self.pcg(w, tau, A0PY)
        PA0PY = PA0PY_1 - Sigma_iX @ (cov @ (Sigma_iX.T @ PA0PY_1))
        AI[0, 0] = float(A0PY @ PA0PY)
        PAPY_1 = self.pcg(w, tau, APY)
        PAPY = PAPY_1 - Sigma_iX @ (cov @ (Sigma_iX.T @ PAPY_1))
        AI[1, 1] = float(APY @ PAPY)
        AI[1, 0] = AI[0, 1] = float(A0PY @ PAPY)
        return YPAPY, trace, AI

    # fitglmmaiRPCG (:867-896)
    def update_tau(self, c, tau0):
        tol = self.p.tol
        YPAPY, trace, AI = self.get_AI_score(c["Y"], c["W"], tau0, c["Sigma_iY"], c["Sigma_iX"], c["cov"])
        Dtau = (YPAPY - trace) / AI
        tau = tau0.copy()
        tau[1] = tau0[1] + Dtau
        tau[tau < tol] = 0
        step = 1.0
        while tau[1] < 0.0:
            step *= 0.5
            tau[1] = tau0[1] + step * Dtau
        tau[tau < tol] = 0
        return tau

    # fitglmmaiRPCG_q (:899-929)
    def update_tau_q(self, c, tau0):
        tol = self.p.tol
        zero_v = tau0 < tol
        YPAPY, trace, AI = self.get_AI_score_q(c["Y"], c["W"], tau0, c["Sigma_iY"], c["Sigma_iX"], c["cov"])
        score = np.array([YPAPY[1] - trace[0], YPAPY[0] - trace[1]])
        Dtau = np.linalg.solve(AI, score)
        tau = tau0 + Dtau
        tau[zero_v & (tau < tol)] = 0
        step = 1.0
        while tau[0] < 0.0 or tau[1] < 0.0:
            step *= 0.5
            tau = tau0 + step * Dtau
            tau[zero_v & (tau < tol)] = 0
        tau[tau < tol] = 0
        return tau

    # saige_fit_AI_PCG_binary (:949-1099) / _quant (:1103-1248)
    def fit(self, tau_in, quant: bool, no_iteration: bool = False):
        """``no_iteration``: the coefficients at the given tau only (:1004-1014)."""
        p, fit0, y = self.p, self.fit0, self.y
        tol, n = p.tol, len(y)
        tol_inv_2 = 1 / (tol * tol)
        eta = fit0.linear_predictors.copy()
        eta0 = eta.copy()
        alpha0 = fit0.coefficients.copy()
        alpha = alpha0.copy()
        tau = np.asarray(tau_in, dtype=np.float64).copy()
        tau0 = tau.copy()
        if p.verbose and not no_iteration:
            print("Initial variance component estimates, tau:")
            print(f"    Sigma_E: {tau[0]:g}, Sigma_G: {tau[1]:g}")
        c = self.get_coeff(tau, alpha0, eta0)
        if no_iteration:
            return dict(coefficients=c["alpha"], tau=tau, linear_predictors=c["eta"], fitted_values=c["mu"],
                        residuals=y - c["mu"], cov=c["cov"], converged=True)
        if quant:
            YPAPY, trace, _ = self.get_AI_score_q(c["Y"], c["W"], tau, c["Sigma_iY"], c["Sigma_iX"], c["cov"])
            tau[0] = max(0.0, tau0[0] + tau0[0] * tau0[0] * (YPAPY[1] - trace[0]) / n)
            tau[1] = max(0.0, tau0[1] + tau0[1] * tau0[1] * (YPAPY[0] - trace[1]) / n)
        else:
            YPAPY, trace, _ = self.get_AI_score(c["Y"], c["W"], tau, c["Sigma_iY"], c["Sigma_iX"], c["cov"])
            tau[1] = max(0.0, tau0[1] + tau0[1] * tau0[1] * (YPAPY - trace) / n)
        cov, mu = c["cov"], c["mu"]
        it = 1
        while it <= p.maxiter:
            if p.verbose:
                print(f"Iteration {it}:")
                print("    tau: (" + ", ".join(f"{v:.7g}" for v in tau) + ")")
                print("    fixed coeff: (" + ", ".join(f"{v:.7g}" for v in alpha) + ")")
            alpha0, tau0, eta0 = c["alpha"], tau.copy(), eta
            for itry in range(1, 12):
                c = self.get_coeff(tau0, alpha0, eta0)
                tau = self.update_tau_q(c, tau0) if quant else self.update_tau(c, tau0)
                if np.max(tau) > tol_inv_2:
                    if itry <= 10:
                        tau0[1] *= 0.5
                        if p.verbose:
                            print(f"    large variance estimate observed, retry ({itry}) ...")
                        continue
                    raise OverflowError("Large variance estimate observed in the iterations, model not converged!")
                break
            cov, alpha, eta, mu = c["cov"], c["alpha"], c["eta"], c["mu"]
            if quant:
                if tau[0] <= 0:
                    raise OverflowError("Sigma_E = 0, model not converged!")
            elif tau[1] == 0:
                break
            if np.max(np.abs(tau - tau0) / (np.abs(tau) + np.abs(tau0) + tol)) < tol:
                break
            it += 1
        c = self.get_coeff(tau, alpha0, eta0)
        cov, alpha, eta, mu = c["cov"], c["alpha"], c["eta"], c["mu"]
        if p.verbose:
            print("Final tau: (" + ", ".join(f"{v:.7g}" for v in tau) + ")")
            print("    fixed coeff: (" + ", ".join(f"{v:.7g}" for v in alpha) + ")")
        return dict(coefficients=alpha, tau=tau, linear_predictors=eta, fitted_values=mu,
                    residuals=y - mu, cov=cov, converged=bool(it <= p.maxiter))

    # saige_calc_var_ratio_binary (:1255-1362) / _quant (:1366-1474)
    def var_ratio(self, tau, obj_noK, codes_of_marker, rand_index, quant: bool):
        p, fit0 = self.p, self.fit0
        fam = fit0.family
        eta, mu = fit0.linear_predictors, fit0.fitted_values
        mu_eta = fam.mu_eta(eta)
        W = mu_eta * mu_eta / fam.variance(mu)
        X1 = obj_noK["X1"]
        Sigma_iX = np.ascontiguousarray(self.solve(W, tau, X1.T).T)
        XSX_inv = _mat_inv(X1.T @ Sigma_iX)
        XXVX_inv, XV = obj_noK["XXVX_inv"], obj_noK["XV"]
        rows: List[tuple] = []
        ratio_cv = p.ratioCVcutoff + 0.1
        num_marker, num_tested, snp_idx = p.num_marker, 0, 0
        while ratio_cv > p.ratioCVcutoff and snp_idx < len(rand_index):
            while num_tested < num_marker and snp_idx < len(rand_index):
                i_snp = int(rand_index[snp_idx])
                snp_idx += 1
                G0 = codes_of_marker(i_snp - 1)
                fin = np.isfinite(G0)
                Num = int(fin.sum())
                AC = float(G0[fin].sum())
                AF = AC / (2 * Num) if Num > 0 else float("nan")
                G0 = np.where(fin, G0, 2 * AF)
                if AF > 0.5:
                    G0 = 2 - G0
                    AC = 2 * Num - AC
                    AF = 1 - AF
                if AC <= 20:
                    continue
                G = G0 - XXVX_inv @ (XV @ G0)
                g = G / math.sqrt(AC)
                Sigma_iG = self.pcg(W, tau, G)
                adj = Sigma_iX @ (XSX_inv @ (X1.T @ Sigma_iG))
                var1 = (float(G @ Sigma_iG) - float(G @ adj)) / AC
                var2 = float(np.sum(g * g)) if quant else float(np.sum(mu * (1 - mu) * g * g))
                num_tested += 1
                rows.append((i_snp, AF, AC, var1, var2, var1 / var2))
                if p.verbose:
                    print(f"{num_tested:6d}, maf: {AF:0.4f}, mac: {AC:g},\tratio: {var1 / var2:0.4f} (var1: {var1:.3g}, var2: {var2:.3g})")
            ratio_cv = _calc_cv(np.array([r[5] for r in rows]))
            if ratio_cv > p.ratioCVcutoff:
                num_marker += 10
        return rows


# ---------------------------------------------------------------------------
# host driver


def _parse_formula(formula: str):
    m = re.match(r"^\s*([A-Za-z_.][\w.]*)\s*~\s*(.+)$", formula)
    if not m:
        raise ValueError("inherits(formula, \"formula\") is not TRUE")
    terms = [t.strip() for t in m.group(2).split("+")]
    if any(not re.match(r"^[A-Za-z_.][\w.]*$", t) and t != "1" for t in terms):
        raise ValueError(f"unsupported term in formula '{formula}' (plain additive numeric covariates only)")
    return m.group(1), [t for t in terms if t != "1"]


def _rank_norm(x: np.ndarray) -> np.ndarray:
    """``.rank_norm`` (R/saige_main.r:66): qnorm((rank(x) - 0.5)/n), average ties."""
    from scipy.stats import norm, rankdata
    return norm.ppf((rankdata(x, method="average") - 0.5) / len(x))


@dataclass
class FittedNullModel(NullModel):
    linear_predictors: Optional[np.ndarray] = None
    residuals: Optional[np.ndarray] = None
    cov: Optional[np.ndarray] = None
    converged: bool = True
    var_ratio_table: Dict[str, np.ndarray] = field(default_factory=dict)
    mu_noK: Optional[np.ndarray] = None
    res_noK: Optional[np.ndarray] = None
    loco_steps: Dict[str, Dict[str, Any]] = field(default_factory=dict)    # per chromosome: IRLS steps, PCG iterations


_DS_NODE = "annotation/format/DS"
_MARKER_PASS = 4096                            # markers per pass: bounded host memory at any M x N


def _marker_filter(nv: np.ndarray, ac: np.ndarray, n_samp: int, maf: float, missing_rate: float) -> np.ndarray:
    """The variant filter of the GRM markers (seqSetFilterCond): per variant ``nv`` samples with a value (int64) and
    ``ac``, the sum of their allele counts or dosages -> af = ac / (2 nv), min(af, 1 - af) >= maf and
    (n_samp - nv) / n_samp <= missing_rate."""
    with np.errstate(invalid="ignore", divide="ignore"):
        af = ac / (2.0 * nv)
    return (np.minimum(af, 1 - af) >= maf) & ((n_samp - nv) / n_samp <= missing_rate)


def _ds_grm_markers(src: GdsFile, sel: np.ndarray, n_all: int, want, var_ids: np.ndarray, maf: float,
                    missing_rate: float, on_gpu: bool):
    """GRM markers of a file without genotypes: the rows of ``annotation/format/DS`` rounded to hard calls
    (``gds.round_dosage_codes``), in passes of ``_MARKER_PASS`` variants.  The stored rows go to the device as they
    are (``sgx_quantize_packed``) when ``on_gpu``, else -- an injected operator, or a node of a class the device
    does not take -- through the numpy statement of the same rule.  ``sel``: the model's samples as indices into
    the file's ``n_all``.  The variant filter (``_marker_filter``) takes the REAL dosages, their count and sum
    (SeqArray's allele frequency on a file without genotypes);
    with ``want`` (a set of variant ids) there is no filter and only those rows are quantised.
    -> (keep_idx, keep_packed): per pass the kept row numbers and their 2-bit rows."""
    from .gds import quantize_dosage_2bit
    nd = src.node(_DS_NODE + "/data")
    dims = tuple(nd.dims or ())
    if len(dims) != 2 or int(dims[1]) != n_all:
        raise ValueError(f"'{_DS_NODE}' should be a [variant, sample] matrix of the file's samples.")
    n_samp = int(sel.size)
    sel_q = None if n_samp == n_all else sel       # (indices in increasing order: all of them = the file's order)
    cls = src.dosage_raw_class(_DS_NODE)
    keep_idx: List[np.ndarray] = []
    keep_packed: List[np.ndarray] = []
    for s0 in range(0, int(dims[0]), _MARKER_PASS):
        s1 = min(s0 + _MARKER_PASS, int(dims[0]))
        loc = None
        if want is not None:
            loc = np.flatnonzero(np.fromiter((int(x) in want for x in var_ids[s0:s1]), dtype=bool, count=s1 - s0))
            if loc.size == 0:
                continue
        if cls is None:                            # (dFloat64, say: decoded by the reader)
            raw, scale, offset = src.dosage_real_range(_DS_NODE, s0, s1), 1.0, 0.0
        else:
            raw, _, scale, offset = src.dosage_raw_range(_DS_NODE, s0, s1)
        if loc is not None:
            raw = raw[loc]
        if on_gpu and cls is not None:
            from ._lib import quantize_packed
            pk, _, _, dv, dsum = quantize_packed(raw, cls, scale, offset, n_samp, sel=sel_q)
        else:
            pk, _, _, dv, dsum = quantize_dosage_2bit(raw, cls, scale, offset, sel=sel_q)
        if loc is None:
            loc = np.flatnonzero(_marker_filter(dv.astype(np.int64), dsum, n_samp, maf, missing_rate))
            pk = np.ascontiguousarray(pk[loc])
        keep_idx.append(loc + s0)
        keep_packed.append(pk)
    return keep_idx, keep_packed


def _load_grm_markers(phenovar: str, covars: List[str], cols: Dict[str, np.ndarray], sids: List[str], gdsfile, maf: float,
                      missing_rate: float, max_num_snp: int, variant_id, seed: int, verbose: bool,
                      use_gpu_counts: bool) -> Dict[str, Any]:
    """Samples and GRM markers of a null-model fit (R/saige_main.r:299-333, R/saige_interaction.r:160-200):
    complete cases in the GDS sample order, the maf / missing-rate filter (or ``variant_id``), then
    ``max_num_snp`` markers drawn by R's ``sample()`` after ``set.seed(seed)``."""
    # complete cases, then the GDS sample order (R/saige_main.r:299-311)
    num = np.column_stack([np.asarray(cols[c], dtype=np.float64) for c in [phenovar] + covars])
    keep = ~np.isnan(num).any(axis=1)
    from .assoc import _open_source
    src = _open_source(gdsfile, verbose)
    gsid = [str(s) for s in src.sample_id()]
    pos = {s: i for i, s in enumerate(sids) if keep[i]}
    sel = [i for i, s in enumerate(gsid) if s in pos]
    if not sel:
        raise ValueError("No common sample.id between 'data' and the GDS file.")
    rows = np.array([pos[gsid[i]] for i in sel])
    yv = num[rows, 0]
    Xc = num[rows, 1:]
    sample_ids = [gsid[i] for i in sel]
    n_samp = len(sel)

    m = _select_grm_markers(src, sel, gsid, maf, missing_rate, max_num_snp, variant_id, seed, verbose, use_gpu_counts)
    return dict(y=yv, Xc=Xc, rows=rows, sample_id=sample_ids, n_samp=n_samp, src=src, **m)


def _select_grm_markers(src, sel: List[int], gsid: List[str], maf: float, missing_rate: float, max_num_snp: int,
                        variant_id, seed: int, verbose: bool, use_gpu_counts: bool) -> Dict[str, Any]:
    """The GRM markers of the samples ``sel`` (increasing indices into the file's samples ``gsid``): the maf /
    missing-rate filter (or ``variant_id``), then ``max_num_snp`` markers drawn by R's ``sample()`` after
    ``set.seed(seed)``.  Shared by the null-model fit and the explicit GRM (grm.py)."""
    from .assoc import GenotypeSource
    n_samp = len(sel)
    # genotypes of the selected samples; variant filter (seqSetFilterCond, :314-321)
    want = None if variant_id is None else set(int(v) for v in variant_id)
    ds_route = False
    keep_idx: List[np.ndarray] = []
    keep_packed: List[np.ndarray] = []
    if isinstance(src, GenotypeSource):
        packed_all, n_all = src.packed, len(gsid)
        var_ids = np.asarray(src.variant_id)
    elif src.has_genotype():                       # (also when a DS node is present: the reference's order)
        packed_all, n_all, _ = src.dosage_alt_packed()
        var_ids = np.asarray(src.read("variant.id"))
    elif src.node(_DS_NODE + "/data", silent=True) is not None:
        # no genotypes: the dosages, rounded to hard calls (R/saige_main.r:395-417, saige_get_sparse)
        if verbose:
            print(f"    using '{_DS_NODE}'")
        var_ids = np.asarray(src.read("variant.id"))
        if variant_id is None and verbose:
            print("Filtering variants:")
        keep_idx, keep_packed = _ds_grm_markers(src, np.asarray(sel), len(gsid), want, var_ids, maf, missing_rate,
                                                use_gpu_counts)
        packed_all, n_all, ds_route = np.zeros((0, 0), dtype=np.uint8), len(gsid), True
    else:
        raise ValueError("'genotype' and 'annotation/format/DS' are not available.")
    packed_all = np.asarray(packed_all)
    gpu_counts = None
    if want is None and n_samp == n_all and use_gpu_counts and not ds_route:
        # all samples selected: the per-variant counts of the filter come from the GPU
        from ._lib import geno_stats_2bit
        gpu_counts = geno_stats_2bit(packed_all, n_all)
    if variant_id is None and verbose and not ds_route:
        print("Filtering variants:")
    same_samples = (n_samp == n_all)
    sel_a = np.asarray(sel)
    CH = _MARKER_PASS
    for s0 in range(0, packed_all.shape[0], CH):
        blk = packed_all[s0:s0 + CH]
        codes = None
        if gpu_counts is not None:
            nv = gpu_counts[0][s0:s0 + CH].astype(np.int64)
            ac = gpu_counts[1][s0:s0 + CH].astype(np.int64)
            loc = np.flatnonzero(_marker_filter(nv, ac, n_samp, maf, missing_rate))
            keep_idx.append(loc + s0)
            keep_packed.append(np.ascontiguousarray(blk[loc]))
            continue
        if want is None or not same_samples:       # (a given variant list on all samples needs no decode)
            codes = unpack_dosage_2bit(blk, n_all)
            if not same_samples:
                codes = codes[:, sel_a]
        if want is None:
            valid = codes != 3
            nv = valid.sum(axis=1)
            ac = np.where(valid, codes, 0).sum(axis=1, dtype=np.int64)
            v = _marker_filter(nv, ac, n_samp, maf, missing_rate)
        else:
            v = np.fromiter((int(x) in want for x in var_ids[s0:s0 + CH]), dtype=bool, count=blk.shape[0])
        loc = np.flatnonzero(v)
        keep_idx.append(loc + s0)
        keep_packed.append(np.ascontiguousarray(blk[loc]) if same_samples else pack_dosage_2bit(codes[loc]))
    rng = RRandom(seed)
    idx = np.concatenate(keep_idx) if keep_idx else np.zeros(0, dtype=np.int64)
    packed = np.concatenate(keep_packed) if keep_packed else np.zeros((0, (n_samp + 3) // 4), dtype=np.uint8)
    del keep_packed
    n_before = idx.size
    if max_num_snp > 0 and idx.size > max_num_snp:
        rng.set_seed(seed)
        pick = np.sort(rng.sample_int(idx.size)[:max_num_snp] - 1)     # sample(which(v), max.num.snp)
        idx, packed = idx[pick], np.ascontiguousarray(packed[pick])
    return dict(packed=packed, idx=idx, var_ids=var_ids, n_before=n_before, rng=rng)


LOCO_MAX_CHROM = 64                            # SGX_GRM_MAX_GROUPS: marker groups of one GRM handle


def _marker_chromosomes(src, idx: np.ndarray):
    """The chromosomes of the GRM markers -> (names in order of first appearance, group id per marker)."""
    from .assoc import GenotypeSource
    chrom = src.chromosome if isinstance(src, GenotypeSource) else src.read("chromosome")
    chrom = np.asarray([str(c) for c in chrom], dtype=object)[idx]
    names: List[str] = []
    seen: Dict[str, int] = {}
    group = np.empty(chrom.size, dtype=np.int32)
    for i, c in enumerate(chrom):
        if c not in seen:
            seen[c] = len(names)
            names.append(c)
        group[i] = seen[c]
    if len(names) < 2:
        raise ValueError(f"loco=True needs GRM markers on more than one chromosome: all {chrom.size} markers are on "
                         f"chromosome '{names[0] if names else ''}'.")
    if len(names) > LOCO_MAX_CHROM:
        raise ValueError(f"loco=True takes at most {LOCO_MAX_CHROM} chromosomes among the GRM markers, found {len(names)}.")
    return names, group


def _fit_loco(fitter: _Fitter, op, operator_factory, packed: np.ndarray, n_samp: int, names: List[str],
              group: np.ndarray, tau: np.ndarray, alpha: np.ndarray, eta: np.ndarray) -> Dict[str, Dict[str, Any]]:
    """Get_Coef_LOCO: for every chromosome, get_coeff at the fitted tau on the GRM without its markers, started
    from the full model's alpha and eta.  On an operator with ``pcg_loco`` all chromosomes run in lockstep and
    share the sweeps of the genotype matrix: an IRLS step is one call of (1 + K) right-hand sides per
    chromosome still iterating, each with its chromosome's weights.  Any other operator (an injected one):
    one operator per chromosome, built from the markers outside it, one after the other."""
    p = fitter.p
    if hasattr(op, "pcg_loco"):
        op.set_groups(group, len(names))

        def solve(act, B, W):
            nb = 1 + fitter.X.shape[1]
            X, its = op.pcg_loco(np.stack([W[c] for c in act]), np.repeat(np.arange(len(act)), nb), tau,
                                 np.vstack([B[c] for c in act]), np.repeat(np.asarray(act), nb), p.maxiterPCG, p.tolPCG)
            return {c: (X[j * nb:(j + 1) * nb], its[j * nb:(j + 1) * nb]) for j, c in enumerate(act)}

        st = fitter.get_coeff_lockstep(tau, alpha, eta, list(range(len(names))), solve)
    else:
        st = {}
        for c in range(len(names)):
            sub = operator_factory(np.ascontiguousarray(packed[group != c]), n_samp)

            def solve(act, B, W, sub=sub):
                S = [sub.pcg(W[act[0]], tau, np.ascontiguousarray(b), p.maxiterPCG, p.tolPCG) for b in B[act[0]]]
                return {act[0]: (np.stack([x for x, _ in S]), [it for _, it in S])}

            try:
                st.update(fitter.get_coeff_lockstep(tau, alpha, eta, [c], solve))
            finally:
                if hasattr(sub, "close"):
                    sub.close()
    return {names[c]: st[c] for c in range(len(names))}


def seqFitNullGLMM_SPA(formula: str, data: Dict[str, Any], gdsfile, trait_type: str = "binary",
                       sample_col: str = "sample.id", maf: float = 0.005, missing_rate: float = 0.01,
                       max_num_snp: int = 1000000, variant_id: Optional[Sequence[int]] = None,
                       inv_norm: bool = True, X_transform: bool = True, tol: float = 0.02, maxiter: int = 20,
                       nrun: int = 30, tolPCG: float = 1e-5, maxiterPCG: int = 500, num_marker: int = 30,
                       tau_init=(0, 0), traceCVcutoff: float = 0.0025, ratioCVcutoff: float = 0.001,
                       geno_sparse: bool = True, num_thread: int = 1, model_savefn: str = "", seed: int = 200,
                       fork_loading: bool = False, verbose: bool = True, operator_factory=None,
                       loco: bool = False, grm_mat=None) -> FittedNullModel:
    """Fit the SAIGE null model ``formula + var(GRM)`` on MI355X.

    ``data``: mapping column -> sequence (a pandas DataFrame works);
    ``gdsfile``: SeqArray GDS path / ``GdsFile`` / ``GenotypeSource``.
    ``operator_factory(packed, n_samp)`` builds the GRM operator; the default is
    the GPU one (``GrmOperator``) -- tests inject the CPU oracle to exercise
    this host logic without a GPU.  A file without ``genotype/data`` gives
    its GRM markers from ``annotation/format/DS``, every dosage rounded to a
    hard call: the reference's default mode (``geno_sparse=TRUE``), which is the
    one implemented -- ``geno_sparse=FALSE`` is not, and the argument is
    accepted for signature compatibility, as are ``num_thread`` and
    ``fork_loading`` (threads only).

    ``loco=True`` adds the leave-one-chromosome-out models (SAIGE's ``LOCO``): after tau is fitted on the whole
    GRM, every chromosome among the GRM markers gets the coefficients and fitted values of the model whose GRM
    leaves that chromosome's markers out (``Get_Coef_LOCO``: ``get_coeff`` at the fitted tau, started from the
    full model), in ``model.loco[chromosome]``; ``seqAssocGLMM_SPA`` then tests the variants of a chromosome
    against its own entry.  tau is not refitted, and the variance ratio stays the single one of the full
    model, as in SAIGE.  The markers must lie on 2 .. 64 chromosomes.  An injected operator without
    ``pcg_loco`` is replaced, per chromosome, by ``operator_factory`` on the markers outside it.

    ``grm_mat`` fits the model on an explicit GRM instead of the implicit one over the markers (SAIGE's
    ``useSparseGRMtoFitNULL``, upstream SAIGEgds 2.x ``grm.mat=``): the ``SparseGRM`` of ``seqFitSparseGRM``, the
    ``(sample_id, K)`` pair of ``seqFitDenseGRM``, or a file either of them wrote (``load_grm``).  Every sample
    of the model must be in the matrix, which is subset and permuted to them; the operator is
    ``ExplicitGrmOperator``, or ``operator_factory(aligned_grm, n_samp)``, and the solves that share (w, tau)
    run as one batched call.  ``gdsfile`` is still needed: the variance-ratio markers and ``variant_id`` come
    from it as without ``grm_mat``.  ``loco=True`` needs the markers and is refused with ``grm_mat``.
    """
    if trait_type not in ("binary", "quantitative"):
        raise ValueError("'arg' should be one of \"binary\", \"quantitative\"")
    phenovar, covars = _parse_formula(formula)
    cols = {k: np.asarray(v) for k, v in dict(data).items()}
    if phenovar not in cols:
        raise ValueError(f"There is no '{phenovar}' in the input data frame.")
    if sample_col in [phenovar] + covars:
        raise ValueError(f"'{sample_col}' should not be in the formula.")
    if sample_col not in cols:
        raise ValueError(f"'{sample_col}' should be one of the columns in 'data'.")
    sids = [str(s) for s in cols[sample_col]]
    if len(set(sids)) != len(sids):
        raise ValueError(f"'{sample_col}' in data should be unique.")
    if grm_mat is not None and loco:
        raise ValueError("loco=True needs the GRM markers: it cannot be combined with 'grm_mat'.")
    if verbose:
        print("SAIGE association analysis:")

    g = _load_grm_markers(phenovar, covars, cols, sids, gdsfile, maf, missing_rate, max_num_snp, variant_id,
                          seed, verbose, use_gpu_counts=operator_factory is None)
    yv, Xc, sample_ids, n_samp = g["y"], g["Xc"], g["sample_id"], g["n_samp"]
    packed, idx, var_ids, n_before, rng = g["packed"], g["idx"], g["var_ids"], g["n_before"], g["rng"]
    n_var = idx.size
    if loco:
        chrom_names, chrom_group = _marker_chromosomes(g["src"], idx)
    if verbose:
        print(f"Fit the null model: {formula} + var(GRM)")
        print(f"    # of samples: {n_samp:,}")
        print(f"    # of variants: {n_var:,}" + (f" (randomly selected from {n_before:,})" if n_before > n_var else ""))

    # design matrix, QR transform (:352-387)
    X = np.column_stack([np.ones(n_samp), Xc])
    X_name = ["(Intercept)"] + covars
    X_qrr = None
    do_tx = bool(X_transform) and X.shape[1] > 1
    if do_tx:
        Q, R = np.linalg.qr(X)
        X_fit = Q * math.sqrt(n_samp)
        X_qrr = R
        if verbose:
            print("Transform on the design matrix with QR decomposition:")
            print("    new formula: y ~ " + " + ".join(f"x_{i}" for i in range(X.shape[1])) + " - 1")
    else:
        X_fit = X

    # GRM operator (saige_store_2b_geno / saige_store_sp_geno), or the one of an explicit matrix
    if grm_mat is not None:
        from .grm import _align_grm_mat
        aligned = _align_grm_mat(grm_mat, sample_ids)
        if operator_factory is None:
            from ._lib import ExplicitGrmOperator
            op = ExplicitGrmOperator(aligned)
        else:
            op = operator_factory(aligned, n_samp)
    elif operator_factory is None:
        from ._lib import GrmOperator
        op = GrmOperator(packed, n_samp)
    else:
        op = operator_factory(packed, n_samp)
    param = _Param(seed=seed, tol=tol, tolPCG=tolPCG, maxiter=int(maxiter), maxiterPCG=int(maxiterPCG),
                   nrun=int(nrun), num_marker=int(num_marker), traceCVcutoff=traceCVcutoff,
                   ratioCVcutoff=ratioCVcutoff, verbose=verbose)
    tau_init = np.nan_to_num(np.asarray(tau_init, dtype=np.float64), nan=0.0)
    tau_init[tau_init < 0] = 0

    def marker(i):
        c8 = unpack_dosage_2bit(packed[i:i + 1], n_samp)[0]
        c = c8.astype(np.float64)
        c[c8 == 3] = np.nan
        return c

    try:
        if trait_type == "binary":
            if len(np.unique(yv)) != 2:
                raise ValueError("The outcome variable has more than 2 categories!")
            fit0 = glm_fit(X_fit, yv, "binomial")
            if verbose:
                print("Initial fixed-effect coefficients:", fit0.coefficients)
            # SPAtest:::ScoreTest_wSaddleApprox_NULL_Model (full-rank X1)
            mu0 = fit0.fitted_values
            V = mu0 * (1 - mu0)
            XV = (X_fit * V[:, None]).T
            XXVX_inv = X_fit @ np.linalg.inv(X_fit.T @ (X_fit * V[:, None]))
            obj_noK = dict(y=yv, mu=mu0, res=yv - mu0, V=V, X1=X_fit, XV=XV, XXVX_inv=XXVX_inv)
            tau = np.array([1.0, 0.5 if tau_init[1] == 0 else tau_init[1]])     # :490-497
            fitter = _Fitter(op, X_fit, yv, fit0, param, rng, batched=grm_mat is not None)
            glmm = fitter.fit(tau, quant=False)
        else:
            y_fit = yv
            if inv_norm:
                f = glm_fit(X_fit, yv, "gaussian")
                resid_sd = float(np.std(f.residuals, ddof=1))
                y_fit = _rank_norm(f.residuals) * resid_sd
                if verbose:
                    print(f"Inverse normal transformation on residuals with standard deviation: {resid_sd}")
            fit0 = glm_fit(X_fit, y_fit, "gaussian")
            mu0 = fit0.fitted_values
            V = np.ones(n_samp)
            obj_noK = dict(y=fit0.y, mu=mu0, res=fit0.y - mu0, V=V, X1=X_fit, XV=X_fit.T.copy(),
                           XXVX_inv=X_fit @ np.linalg.inv(X_fit.T @ X_fit))
            tau = tau_init.copy()
            if tau.sum() == 0:
                tau = np.array([0.5, 0.5])
            Yw = fit0.linear_predictors + (fit0.y - mu0)
            tau = float(np.var(Yw, ddof=1)) * tau / tau.sum()              # :582-589
            fitter = _Fitter(op, X_fit, fit0.y, fit0, param, rng, batched=grm_mat is not None)
            glmm = fitter.fit(tau, quant=True)

        if verbose:
            print("Calculate the average ratio of variances:")
        rng.set_seed(seed)
        rand_index = rng.sample_int(n_var)
        rows_vr = fitter.var_ratio(glmm["tau"], obj_noK, marker, rand_index, quant=(trait_type != "binary"))
        loco_fit = None
        if loco:
            if verbose:
                print(f"Leave-one-chromosome-out models: {len(chrom_names)} chromosomes")
            loco_fit = _fit_loco(fitter, op, operator_factory, packed, n_samp, chrom_names, chrom_group, glmm["tau"],
                                 glmm["coefficients"], glmm["linear_predictors"])
    finally:
        if hasattr(op, "close"):
            op.close()
    rows_vr.sort(key=lambda r: r[0])
    vr = {"id": var_ids[idx][[r[0] - 1 for r in rows_vr]],
          "maf": np.array([r[1] for r in rows_vr]), "mac": np.array([r[2] for r in rows_vr]),
          "var1": np.array([r[3] for r in rows_vr]), "var2": np.array([r[4] for r in rows_vr]),
          "ratio": np.array([r[5] for r in rows_vr])}
    if verbose:
        print(f"    ratio avg. is {np.mean(vr['ratio'])}, sd: {np.std(vr['ratio'], ddof=1)}")

    coef = glmm["coefficients"]
    if do_tx:
        coef = np.linalg.solve(X_qrr, coef * math.sqrt(n_samp))            # :614-622
    model = FittedNullModel(
        trait_type=trait_type, tau=glmm["tau"], fitted_values=glmm["fitted_values"], sample_id=sample_ids,
        var_ratio=vr["ratio"], y=obj_noK["y"], V=obj_noK["V"], X1=obj_noK["X1"], XV=obj_noK["XV"],
        XXVX_inv=obj_noK["XXVX_inv"], coefficients=coef, variant_id=var_ids[idx],
        linear_predictors=glmm["linear_predictors"], residuals=glmm["residuals"], cov=glmm["cov"],
        converged=glmm["converged"], var_ratio_table=vr, mu_noK=obj_noK["mu"], res_noK=obj_noK["res"])
    model.coef_names = X_name
    if loco_fit is not None:
        for name, c in loco_fit.items():
            a = np.linalg.solve(X_qrr, c["alpha"] * math.sqrt(n_samp)) if do_tx else c["alpha"]
            model.loco[name] = dict(coefficients=a, linear_predictors=c["eta"], fitted_values=c["mu"],
                                    residuals=fitter.y - c["mu"], cov=c["cov"])
            model.loco_steps[name] = dict(steps=c["steps"], pcg_iters=c["pcg_iters"])
            if verbose:
                print(f"    chr {name}: {c['steps']} step(s), fixed coeff: (" + ", ".join(f"{v:.7g}" for v in a) + ")")
    if model_savefn:
        from .results import save_model
        if verbose:
            print(f"Save the model to '{model_savefn}'")
        save_model(model, model_savefn)
    if verbose:
        print("Done.")
    return model


def glmmHeritability(modobj, adjust: bool = True) -> float:
    """``glmmHeritability(modobj, adjust)`` (R/saige_main.r:666-691): liability-scale estimate from
    tau; for binary outcomes optionally adjusted by the prevalence (Zhou et al. 2018, Suppl. Table 7)."""
    from .nullmod import load_modobj
    m = load_modobj(modobj)
    if m.trait_type == "binary":
        tau, r = float(m.tau[1]), 1.0
        if adjust:
            y = np.asarray(m.y)
            r = 2.970 + 0.372 * math.log10(float(np.sum(y == 1)) / y.size)
        return tau / (math.pi * math.pi / 3 + tau) * r
    if m.trait_type == "quantitative":
        return float(m.tau[1]) / float(np.sum(m.tau))
    raise ValueError("Invalid 'modobj$trait.type'.")
