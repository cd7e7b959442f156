"""SKAT, the variance-component set test, on MI355X: ``seqAssocGLMM_spaSKAT`` and the mixture p-value
``pchisq_mix``.

The reference has no SKAT (its set tests collapse a unit to one dosage row: burden, ACAT-V, ACAT-O), so nothing here
mirrors reference code and no reference vector pins it: the definition is tied to the project's pinned scan and
burden paths by identities (tests/test_gpu_skat.py).  The flow of a call:

1. the batch loop of the aggregate drivers (``aggregate._prepare`` and ``_run``): per batch of units the scan of the
   batch's variants at thresholds 0 / 0 / 1 for maf, mac and the single-variant p-values;
2. in that loop, ``aggregate.skat_step``: score statistics ``S`` and their covariance ``Phi`` per unit, the weighted
   Gram matrix of the unit's rows on the device's matrix cores;
3. on the host, per unit and weight column: the SPA adjustment of ``Phi`` (binary traits), ``Q = sum w_j^2 S_j^2`` and
   its p-value under the mixture of chi-squares with the eigenvalues of ``diag(w) Phi diag(w)``.

Hard calls are one batch: one ``sgx_scan_2bit`` and one ``sgx_skat_2bit`` for all units.  With ``grm_mat=`` that is one
``sgx_skat_kmat_2bit`` instead: ``Phi`` becomes the covariance under the fitted model on the explicit GRM,
``Phi^K = A' P A``, with no variance ratio.  Dosage input (a format node such as
``annotation/format/DS``, or a ``GenotypeSource(dosage=...)`` that does not reduce to hard calls) is cut into batches
that fit the device: the rows of a batch go to a resident ``DosageBlock`` once, ``blk.scan()`` gives the per-variant
table and ``blk.skat()`` (``sgx_ds_block_skat``) ``S`` and ``Phi`` of the batch's units -- with ``grm_mat=``
``blk.skat_kmat()`` (``sgx_ds_block_skat_kmat``) on one operator for all batches.  With ``collapse_mac=``
 ``aggregate.collapse_step`` runs between steps 1 and 2: one ``sgx_collapse_2bit`` makes a pseudo-variant
of every unit's ultra-rare variants, one more ``sgx_scan_2bit`` scans them; on dosage input one ``blk.collapse()``
(``sgx_ds_block_collapse``) per batch appends them to the resident block, counted and scanned.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import numpy as np

from .aggregate import (NO_DOSAGE_SKAT, AggrParamBeta, _collapse_cols, _dbeta, _prepare, _run, _save, _summary_cols,
                        check_collapse_mac)
from .assoc import GenotypeSource, _open_source, open_scan_input
from .kmat import KmatSolve
from .nullmod import load_modobj, no_loco

LAMBDA_DROP = 1e-10      # eigenvalues at or below this fraction of the largest one are dropped
SERIES_X = 0.05          # |2 t lambda_k| below which a term's functions are summed as power series
LIMIT_T = 1e-150         # |2 t lambda_max| below which the saddlepoint is taken to BE the mean (w -> 0 limit)
_NSER = 24               # terms of those series: 0.05^24 is far below a double's resolution


def _h_u(x: np.ndarray):
    """For x = 2 t lambda (x < 1), without cancellation near x = 0:
         h(x) = [x / (1 - x) + log(1 - x)] / x^2       = sum_{n>=0} (n + 1) / (n + 2) x^n
         u(x) = 1 / (1 - x)^2 - 2 h(x)                 = sum_{n>=1} n (n + 1) / (n + 2) x^n
    so that t q - K(t) = 2 t^2 sum lambda^2 h(x) at the saddlepoint and K''(t) = 2 sum lambda^2 / (1 - x)^2."""
    h, u = np.empty_like(x), np.empty_like(x)
    small = np.abs(x) < SERIES_X
    xs = x[small]
    if xs.size:
        hs, us, p = np.zeros_like(xs), np.zeros_like(xs), np.ones_like(xs)
        for n in range(_NSER):
            hs += (n + 1) / (n + 2) * p
            us += n * (n + 1) / (n + 2) * p
            p = p * xs
        h[small], u[small] = hs, us
    xl = x[~small]
    if xl.size:
        hl = (xl / (1 - xl) + np.log1p(-xl)) / (xl * xl)
        h[~small], u[~small] = hl, 1 / ((1 - xl) * (1 - xl)) - 2 * hl
    return h, u


def pchisq_mix(q: float, lam) -> float:
    """P(sum_k lam_k chi2_1 > q) for lam_k > 0.

    Eigenvalues ``<= 1e-10 * max(lam)`` are dropped.  One eigenvalue left: exact, ``chdtrc(1, q / lam)``.  Otherwise the
    saddlepoint approximation with the cumulant generating function ``K(t) = -1/2 sum log(1 - 2 t lam_k)``:
    ``K'(t^) = q`` is solved on ``t < 1 / (2 max lam)`` by Newton steps kept inside a bracket (bisection when a step
    leaves it), then ``w = sign(t^) sqrt(2 (t^ q - K))``, ``v = t^ sqrt(K'')`` and ``p = 1 - Phi(w + log(v / w) / w)``.

    Near the mean ``q = sum lam`` both ``w`` and ``v`` go to 0 with ``t^``.  They are therefore formed from ``t^`` alone
    (``_h_u``): ``w = 2 t^ sqrt(sum lam^2 h)``, ``v / w`` with ``t^`` cancelled, ``log(v / w) = 1/2 log1p(R)``,
    ``R = sum lam^2 u / (2 sum lam^2 h)`` -- sums of terms of one sign, so the formula keeps its precision down to
    any ``t^ != 0``; terms with ``|2 t^ lam_k| < 0.05`` take the power series of ``h`` and ``u``.  Only where
    ``|2 t^ max lam| < 1e-150`` (in practice: ``q`` equal to the mean) the limit ``log(v / w) / w -> K'''(0) / (6 K''(0)^1.5)``
    is used, ``w = 0``.  The result is continuous and non-increasing in ``q`` through the mean.

    ``q <= 0`` gives 1, an empty ``lam`` (or none positive) NaN.  Accuracy against the exact distribution: DESIGN.md 8b.
    """
    from scipy.special import chdtrc, ndtr
    lam = np.asarray(lam, dtype=np.float64).ravel()
    if lam.size == 0 or not np.all(np.isfinite(lam)) or not math.isfinite(q):
        return float("nan")
    lmax = float(lam.max())
    if not lmax > 0:
        return float("nan")
    if q <= 0:
        return 1.0
    lam = lam[lam > LAMBDA_DROP * lmax]
    if lam.size == 1:
        return float(chdtrc(1.0, q / lam[0]))
    q = float(q)
    mean = float(lam.sum())
    # bracket of the root of K'(t) = sum lam / (1 - 2 t lam) - q: K' is increasing; below the mean every term is
    # under 1 / (2 |t|), so K'(-n / (2 q)) < q; above it the largest term alone reaches q at (1 - lmax / q) / (2 lmax)
    if q > mean:
        lo, hi = 0.0, (1 - lmax / q) / (2 * lmax)
    elif q < mean:
        lo, hi = -lam.size / (2 * q), 0.0
    else:
        lo = hi = 0.0
    t = 0.0
    if lo < hi:
        for _ in range(200):
            d = 1 - 2 * t * lam
            f = float((lam / d).sum()) - q
            if f == 0:
                break
            if f > 0:
                hi = t
            else:
                lo = t
            k2 = 2 * float((lam * lam / (d * d)).sum())
            tn = t - f / k2
            if not (lo < tn < hi):
                tn = 0.5 * (lo + hi)
            if tn == t or abs(tn - t) <= 1e-16 * abs(tn):
                t = tn
                break
            t = tn
    x = 2 * t * lam
    l2 = lam * lam
    if abs(2 * t * lmax) < LIMIT_T:
        k2 = 2 * float(l2.sum())
        z = 8 * float((l2 * lam).sum()) / (6 * k2 ** 1.5)
        return float(ndtr(-z))
    h, u = _h_u(x)
    sh = float((l2 * h).sum())
    w = 2 * t * math.sqrt(sh)
    z = w + 0.5 * math.log1p(float((l2 * u).sum()) / (2 * sh)) / w
    return float(ndtr(-z))


def spa_scale(o, S, var, spa_pval: float) -> np.ndarray:
    """The SPA scale factors of the covariance of score statistics (binary traits): ``o`` the rows of the scan's table,
    ``S`` and ``var`` = Phi_jj of the same variants.  Where a variant went through the SPA stage (p.norm <= spa.pval)
    and it converged with 0 < pval != p.norm and S_j != 0, d_j = S_j^2 / (Phi_jj qchisq(pval_j, 1, upper)), else 1."""
    from scipy.special import chdtri
    S, var = np.asarray(S, dtype=np.float64), np.asarray(var, dtype=np.float64)
    pv, pn, cvg = o[:, 5], o[:, 6], o[:, 7]
    with np.errstate(invalid="ignore"):
        adj = (pn <= spa_pval) & (cvg != 0) & (pv > 0) & (pv != pn) & (S != 0)
    d = np.ones(S.size)
    d[adj] = S[adj] ** 2 / (var[adj] * chdtri(1.0, pv[adj]))
    return d


def device_units(pr):
    """pr.skat, the device step of a batch of units each -> per unit in the units' order (``kept``: its variants in the
    test as rows of pr.out / pr.maf, their scores and covariance, its largest PCG step count; None without ``grm_mat``)."""
    for st in pr.skat:
        for k, (r, a, b) in enumerate(zip(st.kept, st.unit_ptr, st.unit_ptr[1:])):
            yield r, st.score[a:b], st.cov[k], None if st.n_iter is None else (int(st.n_iter[a:b].max()) if r.size else 0)


def unit_walk(pr, units=None):
    """The walk over the units of a call (``units``: what ``device_units`` gives, the default) -> per unit (its number,
    ``kept``, ``S`` and ``Phi`` as float64, ``n_iter``); binary traits: ``Phi`` with the SPA scaling (``spa_scale``)."""
    for u, (r, S, phi, n_iter) in enumerate(device_units(pr) if units is None else units):
        S, phi = np.asarray(S, dtype=np.float64), np.array(phi, dtype=np.float64)
        if pr.binary and r.size:
            sd = np.sqrt(spa_scale(pr.out[r], S, np.diag(phi), pr.sm.spa_pval))
            phi = phi * sd[:, None] * sd[None, :]
        yield u, r, S, phi, n_iter


def _unit_tests(pr, kept, S_of, phi_of):
    """Step 3 of the flow for every unit: ``kept[u]`` the unit's variants (rows of pr.out / pr.maf), ``S_of(u)`` and
    ``phi_of(u)`` their score statistics and covariance -> (Q, pval), [n_units, n_weights] each."""
    nu, nw = len(kept), pr.wbeta.shape[1]
    Q, P = np.full((nu, nw), np.nan), np.full((nu, nw), np.nan)
    for u, r, S, phi, _ in unit_walk(pr, ((r, S_of(u), phi_of(u), None) for u, r in enumerate(kept))):
        if r.size == 0:
            continue
        for i, (a, b) in enumerate(pr.wbeta.T):
            w = _dbeta(pr.maf[r], a, b)
            Q[u, i] = float(np.sum(w * w * S * S))
            wp = phi * w[:, None] * w[None, :]
            if np.all(np.isfinite(wp)) and math.isfinite(Q[u, i]):
                P[u, i] = pchisq_mix(Q[u, i], np.linalg.eigvalsh(wp))
    return Q, P


def aligned_grm_mat(grm_mat, inp, mod):
    """``grm_mat`` as the matrix of the scan's samples in the scan's order, and the model's weights V in that order (the
    drivers that take ``grm_mat=``: SKAT here, the conditional scan in cond.py)."""
    from .grm import _align_grm_mat
    return _align_grm_mat(grm_mat, inp.sample_id()), np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)[inp.ii])


def prepare_skat(what, gdsfile, modobj, units, wbeta, dsnode, spa_pval, var_ratio, parallel, verbose, scanner_factory,
                 ds_budget, grm_mat, tol_pcg, maxiter_pcg, collapse_mac):
    """The head of the SKAT and SKAT-O drivers (``what``: the title a verbose call prints) -> the prepared call.  What
    ``grm_mat=`` refuses without a scanner comes before any row is read (dosage input only where the scanner cannot serve
    it: ``aggregate._dosage_rows``); the solve's tau is the model's, which ``init_nullmod`` hands on as it is."""
    collapse_mac = check_collapse_mac(collapse_mac)
    if not isinstance(dsnode, str):
        raise TypeError("is.character(dsnode) is not TRUE")
    if dsnode != "" and isinstance(gdsfile, GenotypeSource) and gdsfile.packed is not None:
        raise NotImplementedError(NO_DOSAGE_SKAT)
    kmat = None
    if grm_mat is not None:
        if not (parallel is False or parallel is None or (isinstance(parallel, (int, np.integer)) and int(parallel) in (0, 1))):
            raise ValueError("SKAT with 'grm_mat' runs on one GPU: 'parallel' should be FALSE or 1.")
        mod = load_modobj(modobj, False)
        no_loco(mod, "SAIGE SKAT analysis")
        gdsfile = _open_source(gdsfile, False)          # opened once: _prepare goes on with this object
        inp = open_scan_input(gdsfile, mod, dsnode, False)
        kmat = KmatSolve(*aligned_grm_mat(grm_mat, inp, mod), np.asarray(mod.tau, dtype=np.float64), maxiter_pcg, tol_pcg)
    return _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, what, scanner_factory, dsnode, ds_budget,
                    kmat, collapse_mac)


def finish_skat(pr, kept, n_iter, cols, res_savefn, res_compress, verbose) -> Dict[str, Any]:
    """The tail of the SKAT and SKAT-O drivers: the summary columns, ``n.var``, those of ``collapse_mac``, ``n.iter`` (the
    walk's ``n_iter`` per unit), then per weight set the columns ``cols`` (name -> [n_units, n_weights], in the result's
    order; suffix ``.b<a>_<b>`` with more than one weight set); saves the result where asked."""
    ans = _summary_cols(pr)
    ans["n.var"] = np.array([k.size for k in kept], dtype=np.int64)
    _collapse_cols(pr, ans)
    if n_iter[0] is not None:
        ans["n.iter"] = np.array(n_iter, dtype=np.int64)
    for i, nm in enumerate(pr.wb_colnm):
        sfx = f".{nm}" if len(pr.wb_colnm) > 1 else ""
        for c, x in cols.items():
            ans[c + sfx] = x[:, i]
    _save(ans, res_savefn, res_compress, verbose)
    return ans


def seqAssocGLMM_spaSKAT(gdsfile, modobj, units, wbeta=AggrParamBeta, dsnode: str = "", spa_pval: float = 0.05,
                         var_ratio: float = float("nan"), res_savefn: str = "", res_compress: str = "LZMA",
                         parallel=False, verbose: bool = True, verbose_maf: bool = True,
                         scanner_factory=None, ds_budget: Optional[int] = None, grm_mat=None, tol_pcg: float = 1e-5,
                         maxiter_pcg: int = 500, collapse_mac: float = float("nan")) -> Dict[str, Any]:
    """SKAT per unit and weight set (not in the reference; arguments as ``seqAssocGLMM_spaBurden``), on hard calls or
    on dosages (``dsnode``, or a file without ``genotype/data``, or an in-memory dosage matrix that is float64 or holds
    more than hard calls; ``ds_budget``: bytes of resident dosage rows per batch of units).

    Per unit: the variants that pass the scan at thresholds 0 / 0 / 1 with mac > 0; their score statistics ``S`` and
    covariance ``Phi`` (``sgx_skat_2bit``, one call for all units; dosages: ``sgx_ds_block_skat``, one call per batch,
    with the mean and the flip of the scan: ``s / n`` and ``s > n`` of the double sum ``s``).  Binary traits: where a
    variant went through the SPA stage (p.norm <= spa.pval) and it converged with 0 < pval != p.norm and S_j != 0, row
    and column j of ``Phi`` are scaled by the square root of ``d_j = S_j^2 / (Phi_jj qchisq(pval_j, 1, upper))``, so
    that the variant's own chi-square under the scaled variance gives its SPA p-value.  Per weight column (a, b):
    ``w_j = dbeta(maf_j, a, b)``, ``Q = sum w_j^2 S_j^2``, ``pval = pchisq_mix(Q, eigvalsh(diag(w) Phi diag(w)))``.
    Columns: those of the burden driver's summary, ``n.var`` (variants in the test), ``Q`` and ``pval`` (suffix
    ``.b<a>_<b>`` with more than one weight set).  A unit with no variant left gives NaN.

    Two kinds of dosage input are refused with ``NotImplementedError`` (both pinned by
    tests/test_skat.py::test_driver_refuses_dosage_input): a non-empty ``dsnode`` together with an in-memory source of
    packed rows, which has no nodes; and a scanner whose ``dosage_block(...)`` object has no ``skat`` method (checked
    right after the block is made, before any row is read; the scanner is closed).

    ``grm_mat`` (what ``seqFitNullGLMM_SPA(grm_mat=)`` accepts: a ``SparseGRM``, ``(sample_id, K)`` or a file of
    ``load_grm``; every sample of the model must be in it) replaces ``Phi`` by the covariance under the fitted model
    itself, ``Phi^K = A' P A`` with ``Sigma = tau[0] diag(1/V) + tau[1] K`` (``sgx_skat_kmat_2bit``; solves
    to ``tol_pcg`` in at most ``maxiter_pcg`` steps): no variance ratio enters it.  The SPA scale factors are then formed
    against ``Phi^K_jj``; weights, ``Q`` and ``pchisq_mix`` are the same code, and a column ``n.iter`` holds the largest
    PCG step count of the unit.  Dosage input takes ``sgx_ds_block_skat_kmat`` per batch with the scan's
    own mean and flip.  Refused before any row is read: dosage input on a scanner without ``dosage_block`` or whose block
    has no ``skat_kmat`` (``NotImplementedError``; the scanner is closed), a LOCO model, ``parallel`` other than one GPU
    (``ValueError``).

    ``collapse_mac`` (NaN: off, the default; else a number of at least 1, ``ValueError`` below that and ``TypeError`` for
    what is no number; a scanner without ``collapse_2bit`` is refused with ``NotImplementedError`` and closed): the step
    of SAIGE-GENE+, DESIGN.md 8m.  Of a unit's variants in the test those with ``mac <= collapse_mac`` are replaced by
    one pseudo-variant, placed last: per sample the largest minor-allele dosage over them (the code, 2 - code where the
    scan flips the row, 0 where missing), made for all units by one ``sgx_collapse_2bit`` and then scanned, weighted by
    its own maf and entered into ``S``, ``Phi`` (or ``Phi^K``) and the SPA scaling like any variant.  On dosage input
    ``mac`` is the real ``min(s, 2n - s)``, the maximum is over the dosages themselves (2 - x where flipped, 0 where
    missing; strictly ``v > top`` from +0.0) and the pseudo-rows are appended to the resident block by one
    ``sgx_ds_block_collapse`` per batch, each unit counting one more resident row against ``ds_budget``; that needs a
    scanner class that declares ``ds_collapse`` (``Scanner`` does): any other ``scanner_factory`` is refused with
    ``NotImplementedError`` before a scanner is made, a dosage block without ``collapse`` before any row is read.  ``n.var`` counts the entries after collapsing; two more
    columns appear: ``n.collapsed`` (the variants replaced) and ``mac.collapsed`` (the pseudo-variant's minor allele
    count, NaN where nothing was replaced).  The summary columns keep describing the unit's original variants."""
    pr = prepare_skat("SAIGE SKAT analysis:", gdsfile, modobj, units, wbeta, dsnode, spa_pval, var_ratio, parallel, verbose,
                      scanner_factory, ds_budget, grm_mat, tol_pcg, maxiter_pcg, collapse_mac)
    try:
        _run(pr, skat=True)
    finally:
        pr.sc.close()
    kept, S, Phi, n_iter = zip(*device_units(pr))
    Q, P = _unit_tests(pr, kept, S.__getitem__, Phi.__getitem__)      # (the walk scales Phi: it gets the device's own)
    return finish_skat(pr, kept, n_iter, {"Q": Q, "pval": P}, res_savefn, res_compress, verbose)
