"""SNP x SNP interaction test: Python mirror of ``seqGLMM_GxG_spa()``.

Host driver of the reference's R/saige_interaction.r:44-641 and the C++ it calls: for every SNP pair
the GLMM is refitted with the two SNPs as covariates (``saige_fit_AI_PCG_binary``,
src/saige_fitnull.cpp:949-1099) and the product term ``g1 * g2`` is tested with the full saddlepoint
approximation (``saige_GxG_snp_bin`` :1477-1558, ``Saddle_Prob`` src/SPATest.cpp:238-296).

All the cost is PCG solves against the implicit GRM.  The solves that share (w, tau) -- Y and the
columns of X, the Hutchinson vectors of the trace, Sigma_iX with Sigma_iG -- go to the GPU together
(``GrmOperator.pcg_many``): each iteration streams the genotypes once for all of them, and every
column is bit-identical to its single solve, so batching changes no result.
"""
from __future__ import annotations

import math
import re
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .fitnull import _Fitter, _load_grm_markers, _mat_inv, _Param, _parse_formula, glm_fit

# ---------------------------------------------------------------------------
# full saddlepoint approximation (src/SPATest.cpp)

_ROOT_TOL = math.sqrt(math.sqrt(np.finfo(float).eps))     # .Machine$double.eps^0.25
_MAX_ITER = 1000


def _sign(v: float) -> float:
    return v if v != v else (1.0 if v > 0 else (-1.0 if v < 0 else 0.0))


def _korg(t, mu, g):
    return float(np.sum(np.log(1 - mu + mu * np.exp(g * t))))


def _k1_adj(t, mu, g, q):
    return float(np.sum(mu * g / ((1 - mu) * np.exp(-g * t) + mu))) - q


def _k2(t, mu, g):
    e = np.exp(-g * t)
    v = ((1 - mu) * mu * g * g * e) / ((1 - mu) * e + mu) ** 2
    return float(np.sum(v[np.isfinite(v)]))


def _getroot_k1(g_pos, g_neg, mu, g, q, init=0.0, tol=_ROOT_TOL, maxiter=_MAX_ITER):
    """``getroot_K1`` (:92-135) -> (root, converged)."""
    if q >= g_pos or q <= g_neg:
        return math.inf, True
    t = root = init
    k1 = _k1_adj(t, mu, g, q)
    prev_jump = math.inf
    converged = False
    for _ in range(maxiter):
        k2 = _k2(t, mu, g)
        tnew = float(np.float64(t) - np.float64(k1) / np.float64(k2))
        if not math.isfinite(tnew):
            break
        if abs(tnew - t) < tol:
            converged = True
            break
        newk1 = _k1_adj(tnew, mu, g, q)
        if _sign(k1) != _sign(newk1):
            if abs(tnew - t) > prev_jump - tol:
                tnew = t + _sign(newk1 - k1) * prev_jump * 0.5
                newk1 = _k1_adj(tnew, mu, g, q)
                prev_jump *= 0.5
            else:
                prev_jump = abs(tnew - t)
        root = t = tnew
        k1 = newk1
    return root, converged


def _get_saddle_prob(t, mu, g, q):
    """``get_saddle_prob`` (:188-208)."""
    from scipy.special import ndtr
    if not math.isfinite(t):
        return 0.0
    K, k2 = _korg(t, mu, g), _k2(t, mu, g)
    if not (math.isfinite(K) and math.isfinite(k2)):
        return 0.0
    with np.errstate(all="ignore"):
        w = np.float64(_sign(t)) * np.sqrt(np.float64(2 * (t * q - K)))
        v = np.float64(t) * np.sqrt(np.float64(k2))
        z = float(w + np.log(v / w) / w)
    if z > 0:
        return float(ndtr(-z))
    return -float(ndtr(z))


def saddle_prob(q: float, m1: float, var1: float, mu, g, cutoff: float = 2.0):
    """``Saddle_Prob`` (src/SPATest.cpp:238-296): p-value of the score ``q`` from the cumulant
    generating function of sum_i g_i Bernoulli(mu_i), every sample dense.  m1 = sum(mu g),
    var1 = sum(mu (1 - mu) g^2).  Outside |q - m1| / sqrt(var1) < cutoff the saddlepoint p-value is
    used; while it is more than 1000 x smaller than the normal one the cutoff doubles.
    -> (pval, p_noadj, converged)."""
    from scipy.special import chdtrc
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    s = q - m1
    qinv = -s + m1
    p_noadj = float(chdtrc(1, s * s / var1))
    g_pos = g_neg = None
    converged = True
    while True:
        converged = True
        if cutoff < 0.1:
            cutoff = 0.1
        if abs(q - m1) / math.sqrt(var1) < cutoff:
            pval = p_noadj
        else:
            if g_pos is None:
                g_pos, g_neg = float(np.sum(g[g > 0])), float(np.sum(g[g <= 0]))
            with np.errstate(all="ignore"):
                r1, c1 = _getroot_k1(g_pos, g_neg, mu, g, q)
                r2, c2 = _getroot_k1(g_pos, g_neg, mu, g, qinv)
                if c1 and c2:
                    pval = abs(_get_saddle_prob(r1, mu, g, q)) + abs(_get_saddle_prob(r2, mu, g, qinv))
                else:
                    pval = p_noadj
                    converged = False
                    break
        if pval != 0 and p_noadj / pval > 1000:
            cutoff *= 2
        else:
            break
    return pval, p_noadj, converged


# ---------------------------------------------------------------------------
# genotypes of the association file


class DosageMatrix:
    """The matrix form of ``gds_assoc``: dosages [samples x variants] with the sample ids as row names
    and the variant names as column names (``1..ncol`` when not given, as R/saige_interaction.r:113-114)."""

    def __init__(self, dosage, sample_id: Sequence, variant_name: Optional[Sequence] = None):
        self.dosage = np.asarray(dosage, dtype=np.float64)
        if self.dosage.ndim != 2:
            raise ValueError("is.matrix(gds_assoc) is not TRUE")
        if sample_id is None:
            raise ValueError("rownames(gds_assoc) should be sample IDs, if gds_assoc is a matrix.")
        self.sample_id = [str(s) for s in sample_id]
        if len(self.sample_id) != self.dosage.shape[0]:
            raise ValueError("rownames(gds_assoc) should have one sample ID per row")
        nv = self.dosage.shape[1]
        self.variant_name = [str(v) for v in (range(1, nv + 1) if variant_name is None else variant_name)]


def minor_allele_geno(geno) -> np.ndarray:
    """``.minor_allele_geno`` (R/saige_interaction.r:14-25): NA -> the mean, then 2 - g when the mean
    exceeds 1."""
    g = np.array(geno, dtype=np.float64)
    na = np.isnan(g)
    if na.any():
        af = float(np.mean(g[~na])) if (~na).any() else 0.0
        g[na] = af
    if float(np.mean(g)) > 1:
        g = 2 - g
    return g


def _id_str(v) -> str:
    if isinstance(v, (float, np.floating)) and float(v).is_integer():
        return str(int(v))
    return str(v)


class _AssocSource:
    """What the pair loop reads of ``gds_assoc``: per variant id, the dosages of the analysed samples
    (NaN for samples the file lacks), the label and the id column of the result."""

    def __init__(self, gds_assoc, grm_src, sid: List[str], ids: List[Any], verbose: bool):
        from .assoc import GenotypeSource, _open_source
        from .gds import GdsFile
        self.matrix = isinstance(gds_assoc, DosageMatrix)
        if self.matrix:
            src = gds_assoc
            names = {v: j for j, v in enumerate(src.variant_name)}
            self._col = {}
            miss = []
            for v in ids:
                j = names.get(_id_str(v))
                if j is None:
                    miss.append(_id_str(v))
                self._col[_id_str(v)] = j
            file_sid = src.sample_id
        else:
            src = grm_src if gds_assoc is None else _open_source(gds_assoc, verbose)
            vid = np.asarray(src.variant_id if isinstance(src, GenotypeSource) else src.read("variant.id"))
            pos = {int(v): j for j, v in enumerate(vid)}
            self._row = {}
            miss = []
            for v in ids:
                try:
                    j = pos.get(int(v))
                except (TypeError, ValueError):
                    j = None
                if j is None:
                    miss.append(_id_str(v))
                self._row[_id_str(v)] = j
            file_sid = [str(s) for s in src.sample_id()]
            if isinstance(src, GdsFile):
                chrom, posn, allele = src.read("chromosome"), src.read("position"), src.read("allele")
            else:
                chrom, posn = src.chromosome, src.position
                allele = [f"{r},{a}" for r, a in zip(src.ref, src.alt)]
            self._chrom, self._pos, self._allele = chrom, posn, allele
        if miss:
            raise ValueError("No variant ID(s): " + ", ".join(miss))
        self.src = src
        at = {s: i for i, s in enumerate(file_sid)}
        self.i_geno = np.array([at.get(s, -1) for s in sid], dtype=np.int64)
        n_na = int((self.i_geno < 0).sum())
        if n_na:
            if n_na == self.i_geno.size:
                raise ValueError("No common samples in the association GDS file.")
            if verbose:     # (the reference prints the fraction under a percent sign)
                print(f"Missing sample rate in the association GDS file: {n_na / self.i_geno.size:.2f}%")
        self.n_file = len(file_sid)

    def geno(self, v):
        """-> (dosages of the analysed samples with NaN = missing, result id, label)."""
        key = _id_str(v)
        have = self.i_geno >= 0
        out = np.full(self.i_geno.size, np.nan)
        if self.matrix:
            j = self._col[key]
            out[have] = self.src.dosage[self.i_geno[have], j]
            return out, j + 1, v
        j = self._row[key]
        from .assoc import GenotypeSource
        from .gds import unpack_dosage_2bit
        if isinstance(self.src, GenotypeSource):
            if self.src.packed is not None:
                codes = unpack_dosage_2bit(np.asarray(self.src.packed)[j:j + 1], self.n_file)[0]
                row = np.where(codes == 3, np.nan, codes.astype(np.float64))
            else:
                row = np.asarray(self.src.dosage[j], dtype=np.float64)
        else:
            codes = unpack_dosage_2bit(self.src.dosage_alt_packed_range(j, j + 1), self.n_file)[0]
            row = np.where(codes == 3, np.nan, codes.astype(np.float64))
        out[have] = row[self.i_geno[have]]
        label = f"{self._chrom[j]}:{int(self._pos[j])}_" + str(self._allele[j]).replace(",", "_")
        return out, int(v), label


# ---------------------------------------------------------------------------
# per-pair pieces


def _drop_aliased(X: np.ndarray, tol: float = 1e-7) -> np.ndarray:
    """Columns of X that ``lm(y ~ X - 1)`` estimates (the others come out NA): a column whose norm
    after removing the span of the columns kept before it falls under tol times its own norm is
    aliased (LINPACK dqrdc2's limited pivoting, tolerance 1e-7)."""
    keep: List[int] = []
    basis: List[np.ndarray] = []
    for j in range(X.shape[1]):
        v = X[:, j].astype(np.float64).copy()
        n0 = float(np.linalg.norm(v))
        for b in basis:
            v -= (b @ v) * b
        nv = float(np.linalg.norm(v))
        if n0 > 0 and nv >= tol * n0:
            keep.append(j)
            basis.append(v / nv)
    return np.asarray(keep, dtype=np.int64)


def _qr_design(X: np.ndarray) -> np.ndarray:
    Q, _ = np.linalg.qr(X)
    return Q * math.sqrt(X.shape[0])


def _null_model_noK(X1: np.ndarray, y: np.ndarray, fit0) -> Dict[str, np.ndarray]:
    """``SPAtest:::ScoreTest_wSaddleApprox_NULL_Model`` on a full-rank design (the same glm fit)."""
    mu = fit0.fitted_values
    V = mu * (1 - mu)
    XV = (X1 * V[:, None]).T
    XXVX_inv = X1 @ np.linalg.inv(X1.T @ (X1 * V[:, None]))
    return dict(y=y, mu=mu, res=y - mu, V=V, X1=X1, XV=XV, XXVX_inv=XXVX_inv)


def saige_gxg_snp_bin(fitter: _Fitter, fit0, tau, G0: np.ndarray, obj_noK: Dict[str, np.ndarray]) -> Dict[str, Any]:
    """``saige_GxG_snp_bin`` (src/saige_fitnull.cpp:1477-1558): eta and mu of the glm fit, tau of the
    GLMM; Sigma_iX and Sigma_iG are one ``fitter.solve``."""
    from scipy.special import ndtri
    fam = fit0.family
    eta, mu = fit0.linear_predictors, fit0.fitted_values
    mu_eta = fam.mu_eta(eta)
    W = mu_eta * mu_eta / fam.variance(mu)
    tau = np.asarray(tau, dtype=np.float64)
    X1 = obj_noK["X1"]
    y = fit0.y
    G0 = np.asarray(G0, dtype=np.float64)
    n_nonzero = int(np.count_nonzero(G0))
    G = G0 - obj_noK["XXVX_inv"] @ (obj_noK["XV"] @ G0)
    S = fitter.solve(W, tau, np.vstack([X1.T, G[None, :]]))
    Sigma_iX, Sigma_iG = np.ascontiguousarray(S[:-1].T), S[-1]
    adj = Sigma_iX @ (_mat_inv(X1.T @ Sigma_iX) @ (X1.T @ Sigma_iG))
    S_ = float(np.sum((y - mu) * G))
    var1 = float(np.sum(G * Sigma_iG)) - float(np.sum(G * adj))
    var2 = float(np.sum(mu * (1 - mu) * G * G))
    beta = S_ / var1
    q = float(np.sum(y * G))
    m1 = float(np.sum(mu * G))
    qtilde = (q - m1) / math.sqrt(var1) * math.sqrt(var2) + m1
    pval, pnorm, converged = saddle_prob(qtilde, m1, var2, mu, G, 2.0)
    SE = abs(beta / float(ndtri(pval / 2)))
    return {"beta": beta, "SE": SE, "n_nonzero": n_nonzero, "pval": pval, "p.norm": pnorm,
            "converged": bool(converged), "tau_G": float(tau[1])}


# ---------------------------------------------------------------------------
# result table and files


class GxGTable(dict):
    """Result of ``seqGLMM_GxG_spa``: column name -> values in R's column order; ``attrs`` holds
    ``tau_G`` under ``use_approx_tau`` (``attr(rv_ans, "tau_G")``)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.attrs: Dict[str, Any] = {}

    @property
    def nrow(self) -> int:
        return len(next(iter(self.values()))) if self else 0


def _r_num(v) -> str:
    """as.character of a double (15 significant digits), as write.table writes it."""
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "Inf" if v > 0 else "-Inf"
    s = f"{v:.15g}"
    if "e" in s:
        m, e = s.split("e")
        s = f"{m}e{'-' if int(e) < 0 else '+'}{abs(int(e)):02d}"
    return s


def _cells(col, quote: bool) -> List[str]:
    a = np.asarray(col)
    if a.dtype.kind == "b":
        return ["TRUE" if v else "FALSE" for v in a]
    if a.dtype.kind in "iu":
        return [str(int(v)) for v in a]
    if a.dtype.kind == "f":
        return [_r_num(v) for v in a]
    return [f'"{v}"' if quote else str(v) for v in a]


def save_gxg(tab: GxGTable, fn: str):
    """The file formats of R/saige_interaction.r:612-631: .rda/.RData (``save(.x)``), .rds, .txt
    (``write.table(sep="\\t", quote=FALSE)``), .csv (``write.csv``)."""
    from . import results
    if re.search(r"\.(rda|RData)$", fn, re.I):
        raw = b"RDX2\n" + results._HEADER + results._pairlist([(".x", _data_frame_bytes(tab))])
        with open(fn, "wb") as f:
            f.write(results._compress(raw, "ZIP"))
    elif re.search(r"\.rds$", fn, re.I):
        with open(fn, "wb") as f:
            f.write(results._compress(results._HEADER + _data_frame_bytes(tab), "ZIP"))
    elif re.search(r"\.(txt|csv)$", fn, re.I):
        csv = fn.lower().endswith(".csv")
        sep = "," if csv else "\t"
        names = list(tab)
        cols = [_cells(tab[k], csv) for k in names]
        with open(fn, "w") as f:
            f.write(sep.join(f'"{k}"' if csv else k for k in names) + "\n")
            for r in range(tab.nrow):
                f.write(sep.join(c[r] for c in cols) + "\n")
    else:
        raise ValueError("Unknown format of the output file, and it should be RData or RDS.")


def _data_frame_bytes(tab: GxGTable) -> bytes:
    from . import results
    attrs = [("tau_G", results._vector(np.array([float(tab.attrs["tau_G"])])))] if "tau_G" in tab.attrs else []
    return results._data_frame(dict(tab), extra_attrs=attrs)


# ---------------------------------------------------------------------------
# driver


def _snp_pair_columns(snp_pair) -> Dict[str, np.ndarray]:
    cols = {str(k): np.asarray(v) for k, v in dict(snp_pair).items()}
    if len(cols) < 2 or len(next(iter(cols.values()))) == 0:
        raise ValueError("is.data.frame(snp_pair), ncol(snp_pair) >= 2L, nrow(snp_pair) > 0L is not TRUE")
    n = len(next(iter(cols.values())))
    if any(len(v) != n for v in cols.values()):
        raise ValueError("the columns of 'snp_pair' differ in length")
    return cols


def _is_na(v) -> bool:
    if v is None:
        return True
    try:
        return bool(np.isnan(v))
    except TypeError:
        return False


def seqGLMM_GxG_spa(formula: str, data: Dict[str, Any], gds_grm, gds_assoc, snp_pair,
                    trait_type: str = "binary", sample_col: str = "sample.id", maf: float = 0.005,
                    missing_rate: float = 0.01, max_num_snp: int = 1000000,
                    variant_id: Optional[Sequence[int]] = None, inv_norm: bool = True, X_transform: bool = True,
                    tol: float = 0.02, maxiter: int = 20, nrun: int = 30, tolPCG: float = 1e-5,
                    maxiterPCG: int = 500, tau_init=(0, 0), use_approx_tau: bool = False, glm_threshold=False,
                    traceCVcutoff: float = 0.0025, ratioCVcutoff: float = 0.001, geno_sparse: bool = True,
                    num_thread: int = 1, model_savefn: str = "", seed: int = 200, fork_loading: bool = False,
                    verbose: bool = True, verbose_detail: bool = True, operator_factory=None,
                    batch_solves: bool = True) -> GxGTable:
    """GxG interaction test of SNP pairs with the SAIGE GLMM (binary traits).

    ``gds_grm``: GDS path / ``GdsFile`` / ``GenotypeSource`` of the GRM markers; ``gds_assoc``: the
    same kinds, ``None`` (use ``gds_grm``) or a ``DosageMatrix``; ``snp_pair``: mapping of columns (a
    pandas DataFrame works), the first two the variant ids of a pair, further columns are appended to
    the result.  ``operator_factory(packed, n_samp)`` builds the GRM operator (default: the GPU
    ``GrmOperator``); ``batch_solves=False`` solves one vector at a time (same results).  ``inv_norm``,
    ``X_transform`` (for the pairs), ``ratioCVcutoff``, ``num_thread`` and ``fork_loading`` do not change
    what the reference computes for binary traits and are accepted for signature compatibility.  A
    ``gds_grm`` file without ``genotype/data`` gives its markers from ``annotation/format/DS``, every dosage
    rounded to a hard call: the reference's default mode (``geno_sparse=TRUE``,
    R/saige_interaction.r:223-236), the one implemented; ``geno_sparse`` itself is accepted and not read.
    Returns a ``GxGTable`` (column -> values, R's column order)."""
    if trait_type not in ("binary", "quantitative"):
        raise ValueError("'arg' should be one of \"binary\", \"quantitative\"")
    if not verbose:
        verbose_detail = False
    pairs = _snp_pair_columns(snp_pair)
    pnames = list(pairs)
    c1, c2 = pairs[pnames[0]], pairs[pnames[1]]
    if any(_is_na(v) for col in pairs.values() for v in col):
        raise ValueError("'snp_pair' should not have missing values.")
    if any(_id_str(a) == _id_str(b) for a, b in zip(c1, c2)):
        raise ValueError("'snp_pair' should not have the same variant in a pair.")
    if verbose:
        print("SAIGE association analysis on the GxG interaction:")

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

    g = _load_grm_markers(phenovar, covars, cols, sids, gds_grm, maf, missing_rate, max_num_snp, variant_id,
                          seed, verbose, use_gpu_counts=operator_factory is None)
    y, Xc, sid, n_samp, packed, rng = g["y"], g["Xc"], g["sample_id"], g["n_samp"], g["packed"], g["rng"]
    n_var = int(g["idx"].size)
    if verbose:
        print(f"Fit the null model: {formula} + var(GRM)")
        print(f"    # of samples: {n_samp:,}")
        print(f"    # of variants: {n_var:,}" + (f" (randomly selected from {g['n_before']:,})"
                                                 if g["n_before"] > n_var else ""))

    ids = list(dict.fromkeys([*c1.tolist(), *c2.tolist()]))
    assoc = _AssocSource(gds_assoc, g["src"], sid, ids, verbose)
    if trait_type == "quantitative":
        raise NotImplementedError("Not implement yet.")
    if len(np.unique(y)) != 2:
        raise ValueError("The outcome variable has more than 2 categories!")

    if operator_factory is None:
        from ._lib import GrmOperator
        op = GrmOperator(packed, n_samp)
    else:
        op = operator_factory(packed, n_samp)
    param = _Param(seed=seed, tol=tol, tolPCG=tolPCG, maxiter=int(maxiter), maxiterPCG=int(maxiterPCG),
                   nrun=int(nrun), num_marker=1, traceCVcutoff=traceCVcutoff, ratioCVcutoff=ratioCVcutoff,
                   verbose=verbose_detail)
    tau_init = np.nan_to_num(np.asarray(tau_init, dtype=np.float64), nan=0.0)
    tau_init[tau_init < 0] = 0
    ori_X = np.column_stack([np.ones(n_samp), Xc])

    def fitter(X, fit0):
        return _Fitter(op, X, y, fit0, param, rng, batched=batch_solves)

    def glmm_tau(tau):
        t = np.array([1.0, 0.0])
        t[1] = 0.5 if tau[1] == 0 else tau[1]
        return t

    try:
        if use_approx_tau:
            if verbose:
                print("Fitting the model without the SNP markers to find the initial tau:")
            X = ori_X
            if X.shape[1] > 1 and X_transform:
                X = _qr_design(X[:, _drop_aliased(X)])
            fit0 = glm_fit(X, y, "binomial")
            glmm = fitter(X, fit0).fit(glmm_tau(tau_init), quant=False)
            tau_init = np.asarray(glmm["tau"], dtype=np.float64)
        else:
            tau_init = glmm_tau(tau_init)
        if verbose and use_approx_tau:
            print(f"Use tau for the interaction: ({tau_init[0]:g}, {tau_init[1]:g})")
        if glm_threshold is None or (isinstance(glm_threshold, float) and math.isnan(glm_threshold)):
            glm_threshold = False
        if glm_threshold is True:
            glm_threshold = 0.01
        use_glm = glm_threshold is not False
        if verbose and use_glm:
            print(f"GLM p-value threshold: {glm_threshold:g}")
        if verbose:
            print(f"Testing the interaction, # of SNP pairs: {len(c1)}")

        rows: List[Dict[str, Any]] = []
        out = GxGTable()
        for ii, (v1, v2) in enumerate(zip(c1.tolist(), c2.tolist())):
            if verbose:
                print(f"==> {ii + 1}: SNP {_id_str(v1)} x SNP {_id_str(v2)} <==")
            r1, id1, s1 = assoc.geno(v1)
            g1 = minor_allele_geno(r1)
            maf1 = float(np.mean(g1)) * 0.5
            r2, id2, s2 = assoc.geno(v2)
            g2 = minor_allele_geno(r2)
            maf2 = float(np.mean(g2)) * 0.5
            if verbose:
                print(f"    SNP1 ({s1}), MAF: {maf1:.5g}")
                print(f"    SNP2 ({s2}), MAF: {maf2:.5g}")
            X = np.column_stack([ori_X, g1, g2])
            X_new = _qr_design(X[:, _drop_aliased(X)])
            fit0 = glm_fit(X_new, y, "binomial")
            obj_noK = _null_model_noK(X_new, y, fit0)
            pv = pv2 = None
            run_glmm = True
            if use_glm:
                f = fitter(X_new, fit0)
                glmm = f.fit(np.array([1.0, 0.0]), quant=False, no_iteration=True)
                d = saige_gxg_snp_bin(f, fit0, glmm["tau"], g1 * g2, obj_noK)
                pv, pv2 = d["pval"], d["p.norm"]
                d["pval"] = d["p.norm"] = math.nan
                d["p.glm"], d["p.glm.norm"] = pv, pv2
                run_glmm = math.isfinite(pv) and pv <= glm_threshold
                if verbose_detail:
                    print(f"    glm p-value: {pv:g} " + ("<= threshold" if run_glmm else "> threshold (skip glmm)"))
            if run_glmm:
                f = fitter(X_new, fit0)
                glmm = f.fit(tau_init.copy(), quant=False, no_iteration=use_approx_tau)
                d = saige_gxg_snp_bin(f, fit0, glmm["tau"], g1 * g2, obj_noK)
                if pv is not None and not math.isnan(pv):
                    d["p.glm"], d["p.glm.norm"] = pv, pv2
            if verbose:
                print(f"    Nonzero #: {d['n_nonzero']}, beta: {d['beta']:.6g}, SE: {d['SE']:.6g}, "
                      f"pval: {d['pval']:.6g}, pnorm: {d['p.norm']:.6g}, tau_G: {d['tau_G']:.5g}")
            rows.append(dict(id1=id1, snp1=str(s1), maf1=maf1, id2=id2, snp2=str(s2), maf2=maf2, **d))
            out = _table(rows, pairs, pnames)
            if use_approx_tau:
                out.attrs["tau_G"] = float(tau_init[1])
            if model_savefn:
                if verbose:
                    print(f"    Save the results to '{model_savefn}'")
                save_gxg(out, model_savefn)
    finally:
        if hasattr(op, "close"):
            op.close()
    if verbose:
        print("Done.")
    return out


def _table(rows: List[Dict[str, Any]], pairs: Dict[str, np.ndarray], pnames: List[str]) -> GxGTable:
    names = list(rows[0])
    for r in rows[1:]:               # (rbind: the glm columns of a later row extend the table)
        names += [k for k in r if k not in names]
    t = GxGTable()
    for k in names:
        vals = [r.get(k, math.nan) for r in rows]
        if k in ("id1", "id2", "n_nonzero"):
            t[k] = np.asarray(vals, dtype=np.int64) if all(isinstance(v, (int, np.integer)) for v in vals) \
                else np.asarray(vals)
        elif k in ("snp1", "snp2"):
            t[k] = np.asarray([str(v) for v in vals])
        elif k == "converged":
            t[k] = np.asarray(vals, dtype=bool)
        else:
            t[k] = np.asarray(vals, dtype=np.float64)
    for k in pnames[2:]:
        t[k] = np.asarray(pairs[k])[:len(rows)]
    return t
