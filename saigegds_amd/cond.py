"""Conditional association scan on MI355X: ``seqAssocGLMM_SPA_cond`` tests every variant given a set of conditioning
(lead) variants, ``cond_tests`` is its host algebra.

The reference has no conditional analysis (SAIGE proper has ``--condition``), so nothing here mirrors reference code
and no reference vector pins it: the definition is tied to the project's pinned scan and SKAT paths by identities
(DESIGN.md 8b "Conditional analysis", tests/test_gpu_cond.py).  With the score statistics ``S`` and their covariance
``Phi`` as ``sgx_skat_2bit`` defines them, the test of variant j given the set C is the score test of the part of
``G_j`` that the conditioning variants do not explain:

    T = S_j - Phi_jC Phi_CC^-1 S_C,    V = Phi_jj - Phi_jC Phi_CC^-1 Phi_Cj,    chi-square = T^2 / V.

The flow of a call: the conditioning rows are scanned at thresholds 0 / 0 / 1 and installed with ``sgx_cond_set``
(``S_C``, ``Phi_CC``); then per block of variants the rows go to the device once, ``sgx_scan_2bit_dev`` makes the
single-variant table, the dosage tables are built on the device from its ``AF`` column, ``sgx_cond_2bit_dev`` makes
``S_j``, ``Phi_jj`` and ``Phi_jC`` of every row, and one download brings everything back.

Dosage input -- a format node such as ``annotation/format/DS``, or a ``GenotypeSource(dosage=...)`` -- takes the
resident dosage block of the aggregate drivers (``DosageBlock``): the conditioning rows are loaded into a block of
their own, scanned and installed from there (``sgx_ds_block_cond_set``); then per batch of rows that fits
``aggregate.DS_BUDGET`` bytes one load, ``scan()``, and ``cond(flip, mean)`` (``sgx_ds_block_cond``) with the scan's own
imputation and flip, formed from the load's counts as the SKAT driver forms them.

``grm_mat=`` replaces ``Phi`` by the covariance under the fitted model on the explicit GRM, ``Phi^K`` of
``seqAssocGLMM_spaSKAT(grm_mat=)``: the set is installed with ``sgx_cond_kmat_set``, which solves its
columns once, and per block the rows are scanned and go through ``sgx_cond_kmat_2bit`` from host memory.  On dosage
input the same two steps are the block's ``cond_kmat_set`` and ``cond_kmat``
(``sgx_ds_block_cond_kmat_set`` / ``sgx_ds_block_cond_kmat``) on the resident rows.
"""
from __future__ import annotations

import collections
import contextlib
import math
import re
from typing import Any, Dict, Optional

import numpy as np

from . import aggregate
from .assoc import (BLOCK_SIZE, GenotypeSource, ScanInput, _open_source, _pretty, assemble_result,
                    check_scan_args, finish_result, open_scan_input, require_device)
from .kmat import NO_DOSAGE_KMAT, KmatSolve
from .nullmod import ModelError, NullModel, init_nullmod, load_modobj, no_loco
from .skat import aligned_grm_mat, spa_scale

COND_MAX = 16             # SGX_COND_MAX: conditioning variants of one call
COND_COLLINEAR = 1e-6     # V <= this fraction of Phi_jj: the variant is taken to be explained by the set (a definition:
#                           Phi is good to ~1e-10 of itself, so anything near 1e-8 is noise)


def _cholesky(a: np.ndarray) -> np.ndarray:
    """Lower Cholesky factor; ValueError where a pivot is not above COND_COLLINEAR times its diagonal entry."""
    c = a.shape[0]
    L = np.zeros((c, c))
    for k in range(c):
        piv = a[k, k] - float(L[k, :k] @ L[k, :k])
        if not (a[k, k] > 0 and piv > COND_COLLINEAR * a[k, k]):
            raise ValueError("The conditioning variants are collinear.")
        L[k, k] = math.sqrt(piv)
        L[k + 1:, k] = (a[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def cond_tests(S, var, cov, S_C, Phi_CC, d=None, d_C=None):
    """Conditional score tests, vectorised over rows: ``S`` [m], ``var`` = Phi_jj [m], ``cov`` = Phi_jC [m, C] of the
    scanned rows, ``S_C`` [C] and ``Phi_CC`` [C, C] of the conditioning set; ``d`` [m] / ``d_C`` [C]: the SPA scale
    factors (``skat.spa_scale``), Phi~ = D^1/2 Phi D^1/2.  -> (beta, SE, pval):

        T = S_j - Phi~_jC Phi~_CC^-1 S_C,  V = Phi~_jj - Phi~_jC Phi~_CC^-1 Phi~_Cj,
        beta = T / V,  SE = 1 / sqrt(V),  pval = chdtrc(1, T^2 / V).

    A row with ``V <= COND_COLLINEAR * Phi~_jj`` (a variant of the set itself, say) gets NaN in all three.  ``Phi~_CC``
    is factorised once by Cholesky; if a pivot is at or below COND_COLLINEAR times its diagonal entry, ``ValueError``."""
    from scipy.linalg import solve_triangular
    from scipy.special import chdtrc
    S, var = np.asarray(S, dtype=np.float64), np.asarray(var, dtype=np.float64)
    S_C, Phi_CC = np.asarray(S_C, dtype=np.float64), np.asarray(Phi_CC, dtype=np.float64)
    c = S_C.size
    cov = np.asarray(cov, dtype=np.float64).reshape(S.size, c)
    if Phi_CC.shape != (c, c) or var.shape != S.shape:
        raise ValueError("cond_tests: inconsistent shapes")
    if d is not None:
        d = np.asarray(d, dtype=np.float64)
        var, cov = var * d, cov * np.sqrt(d)[:, None]
    if d_C is not None:
        sc_ = np.sqrt(np.asarray(d_C, dtype=np.float64))
        cov, Phi_CC = cov * sc_[None, :], Phi_CC * sc_[:, None] * sc_[None, :]
    if not np.all(np.isfinite(Phi_CC)) or not np.all(np.isfinite(S_C)):
        raise ValueError("The conditioning variants are collinear.")
    L = _cholesky(Phi_CC)
    z = solve_triangular(L, S_C, lower=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        Y = solve_triangular(L, np.where(np.isfinite(cov), cov, 0.0).T, lower=True)      # [C, m]
        T = S - Y.T @ z
        V = var - np.sum(Y * Y, axis=0)
        ok = np.isfinite(cov).all(axis=1) & np.isfinite(S) & (V > COND_COLLINEAR * var)
        beta, se, p = (np.full(S.size, np.nan) for _ in range(3))
        beta[ok], se[ok] = T[ok] / V[ok], 1.0 / np.sqrt(V[ok])
        p[ok] = chdtrc(1.0, T[ok] * T[ok] / V[ok])
    return beta, se, p


def _tables(af, valid):
    """Dosage tables of the rows on the rows' device (torch): m = 2 AF, flipped where AF > 0.5 -- {0, 1, 2, m} or
    {2, 1, 0, 2 - m}, the imputation and flip of the scan itself; NaN where the row is not valid.  The tables are those
    of ``aggregate.dosage_tables`` (the definition on the host), restated here because AF stays on the device."""
    import torch
    m = 2 * af
    z = torch.zeros_like(m)
    lut = torch.where((af > 0.5)[:, None], torch.stack([z + 2, z + 1, z, 2 - m], dim=1), torch.stack([z, z + 1, z + 2, m], dim=1))
    return torch.where(valid[:, None], lut, torch.full_like(lut, float("nan"))).contiguous()


_NO_DOSAGE = "Conditional analysis on dosage input is not implemented."
_NO_DOSAGE_KMAT = NO_DOSAGE_KMAT.format("Conditional analysis")

# a route's result (res: _scan_hard); n_iter: the PCG steps of every row's column, None without ``grm_mat``
CondScan = collections.namedtuple("CondScan", "res out_c S_C Phi_CC n_iter")


def _set_phase(sc, cond_ids, thresholds, scan_set, install):
    """The conditioning set of every route, at thresholds 0 / 0 / 1: ``scan_set()`` -> (its scan table, valid flags, what
    ``install`` needs), the check of the set, ``install(out_c, ...)`` -> (S_C, Phi_CC, ...); the call's thresholds return."""
    sc.set_thresholds(0.0, 0.0, 1.0, thresholds[3])
    out_c, valid_c, *more = scan_set()
    for k, v in enumerate(cond_ids):
        if not valid_c[k] or not out_c[k, 1] > 0:
            raise ValueError(f"`condition`: variant {v!r} has no valid genotype or is monomorphic.")
    S_C, Phi_CC = install(out_c, *more)[:2]
    sc.set_thresholds(*thresholds)
    return out_c, S_C, Phi_CC


def _set_2bit(sc, inp: ScanInput, cidx, cond_ids, thresholds, install):
    """``_set_phase`` of the two hard-call routes: ``install(rows_c, lut_c)`` is ``cond_set`` or ``cond_kmat_set``."""
    import torch
    nb = (inp.n_samp + 3) // 4

    def scan_set():
        rows_c = np.ascontiguousarray(np.concatenate([inp.packed_rows(i, i + 1)[:, :nb] for i in cidx]))
        return (*sc.scan_2bit(rows_c), rows_c)

    def put(out_c, rows_c):
        return install(rows_c, _tables(torch.from_numpy(out_c[:, 0].copy()), torch.ones(len(cidx), dtype=torch.bool)).numpy())
    return _set_phase(sc, cond_ids, thresholds, scan_set, put)


def _scan_hard(sc, inp: ScanInput, cidx, cond_ids, thresholds) -> CondScan:
    """The hard-call route: 2-bit rows, resident on the device per block -> res [n_var, 8 + 3 + C]: the scan table, valid,
    S_j, Phi_jj, Phi_jC; the set's scan table, S_C, Phi_CC."""
    import torch
    n_samp, n_var, read_rows = inp.n_samp, inp.n_var, inp.packed_rows
    dev = torch.device(getattr(sc, "torch_device", "cuda"))
    nb = (n_samp + 3) // 4
    out_c, S_C, Phi_CC = _set_2bit(sc, inp, cidx, cond_ids, thresholds, sc.cond_set)

    # the scan, by blocks
    C = len(cidx)
    stride = sc.row_stride()
    res = np.empty((n_var, 8 + 3 + C), dtype=np.float64)
    for off in range(0, n_var, BLOCK_SIZE):
        end = min(n_var, off + BLOCK_SIZE)
        m = end - off
        host = np.zeros((m, stride), dtype=np.uint8)
        host[:, :nb] = read_rows(off, end)[:, :nb]
        rows = torch.from_numpy(host).to(dev)                       # the one upload
        out8 = torch.empty((m, 8), dtype=torch.float64, device=dev)
        valid = torch.zeros(m, dtype=torch.uint8, device=dev)
        score, var = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
        cov = torch.empty((m, C), dtype=torch.float64, device=dev)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        sc.scan_2bit_dev(rows.data_ptr(), stride, m, out8.data_ptr(), valid.data_ptr())
        sc.sync()
        lut = _tables(out8[:, 0], valid != 0)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        sc.cond_2bit_dev(rows.data_ptr(), stride, m, lut.data_ptr(), score.data_ptr(), var.data_ptr(), cov.data_ptr())
        sc.sync()
        res[off:end] = torch.cat([out8, valid.to(torch.float64)[:, None], score[:, None], var[:, None], cov],
                                 dim=1).cpu().numpy()              # the one download
    return CondScan(res, out_c, S_C, Phi_CC, None)


def _scan_kmat(sc, inp: ScanInput, cidx, cond_ids, thresholds, kmat: KmatSolve) -> CondScan:
    """The hard-call route on an explicit GRM: ``Phi^K`` for ``Phi``, the rows from host memory per block."""
    import torch
    n_samp, n_var, read_rows = inp.n_samp, inp.n_var, inp.packed_rows
    nb = (n_samp + 3) // 4
    res = np.empty((n_var, 8 + 3 + len(cidx)), dtype=np.float64)
    n_iter = np.zeros(n_var, dtype=np.int64)
    with kmat.operator(sc) as op:
        out_c, S_C, Phi_CC = _set_2bit(sc, inp, cidx, cond_ids, thresholds,
                                       lambda rows_c, lut_c: sc.cond_kmat_set(op, rows_c, lut_c, *kmat.args))
        for off in range(0, n_var, BLOCK_SIZE):
            end = min(n_var, off + BLOCK_SIZE)
            rows = np.ascontiguousarray(read_rows(off, end)[:, :nb])
            out8, valid = sc.scan_2bit(rows)
            lut = _tables(torch.from_numpy(out8[:, 0].copy()), torch.from_numpy(valid != 0)).numpy()
            score, var, cov, it = sc.cond_kmat(op, rows, lut)      # a row that failed the thresholds: NaN table, no solve
            res[off:end, :8], res[off:end, 8], res[off:end, 9], res[off:end, 10], res[off:end, 11:] = out8, valid, score, var, cov
            n_iter[off:end] = it
    return CondScan(res, out_c, S_C, Phi_CC, n_iter)


def _scan_dosage(sc, inp: ScanInput, stored, cidx, cond_ids, thresholds, kmat: Optional[KmatSolve] = None) -> CondScan:
    """The dosage route, from resident dosage blocks -- with ``kmat`` the set by the block's ``cond_kmat_set`` and the rows
    by its ``cond_kmat``, on one operator.  A row that failed the thresholds gets a NaN mean there: no solve."""
    read_rows, ds_dtype, n_samp, n_var = inp.dosage_reader(stored), inp.ds_dtype, inp.n_samp, inp.n_var

    refusal = _NO_DOSAGE if kmat is None else _NO_DOSAGE_KMAT
    make = getattr(sc, "dosage_block", None)
    if make is None:
        raise NotImplementedError(refusal)
    C = len(cidx)
    order = np.argsort(cidx)                           # the readers take ascending indices
    rank = np.argsort(order).astype(np.int32)          # conditioning variant k is row rank[k] of its block
    n_iter = None if kmat is None else np.zeros(n_var, dtype=np.int64)
    with contextlib.ExitStack() as stack:
        blk = stack.enter_context(make(ds_dtype, C))
        if not hasattr(blk, "cond" if kmat is None else "cond_kmat"):
            raise NotImplementedError(refusal)
        op = None if kmat is None else stack.enter_context(kmat.operator(sc))

        def scan_set():
            n, s, _ = aggregate.load_rows(blk, read_rows(np.asarray(cidx, dtype=np.int64)[order]))
            out_c, valid_c = blk.scan()
            return out_c[rank], valid_c[rank], n, s

        def install(out_c, n, s):
            fl, mean = aggregate.flip_mean(n, s)
            if kmat is None:
                return blk.cond_set(rank, fl[rank], mean[rank])
            return blk.cond_kmat_set(op, rank, fl[rank], mean[rank], *kmat.args)
        out_c, S_C, Phi_CC = _set_phase(sc, cond_ids, thresholds, scan_set, install)
        blk.close()                                    # the set is the scanner's: the rows' block takes the memory
        per = int(max(1, min(n_var, aggregate.DS_BUDGET // aggregate.ds_row_bytes(ds_dtype, n_samp))))
        res = np.empty((n_var, 8 + 3 + C), dtype=np.float64)
        blk = stack.enter_context(make(ds_dtype, per))
        for off in range(0, n_var, per):
            end = min(n_var, off + per)
            n, s, _ = aggregate.load_rows(blk, read_rows(np.arange(off, end, dtype=np.int64)))      # the one upload
            out8, valid = blk.scan()
            fl, mean = aggregate.flip_mean(n, s)
            if kmat is None:
                score, var, cov = blk.cond(fl, mean)
            else:
                score, var, cov, n_iter[off:end] = blk.cond_kmat(op, fl, np.where(valid != 0, mean, np.nan))
            res[off:end, :8], res[off:end, 8], res[off:end, 9], res[off:end, 10], res[off:end, 11:] = out8, valid, score, var, cov
    return CondScan(res, out_c, S_C, Phi_CC, n_iter)


def seqAssocGLMM_SPA_cond(gdsfile, modobj: Any, condition, maf: float = float("nan"), mac: float = 10,
                          missing: float = 0.1, spa_pval: float = 0.05, var_ratio: float = float("nan"),
                          res_savefn: str = "", res_compress: str = "LZMA", verbose: bool = True, dsnode: str = "",
                          scanner_factory=None, grm_mat=None, tol_pcg: float = 1e-5,
                          maxiter_pcg: int = 500) -> Optional[Dict[str, Any]]:
    """Single-variant scan of every variant given the variants ``condition`` (not in the reference).

    ``condition``: 1 to 16 distinct values of the file's ``variant.id`` (of ``GenotypeSource.variant_id``); the other
    arguments as ``seqAssocGLMM_SPA``.  Hard calls (``genotype/data`` or an in-memory source of packed rows) or dosages
    (a non-empty ``dsnode``, a file without ``genotype/data`` -- then ``annotation/format/DS`` --, or an in-memory source
    of uint8 / int32 / float64 dosages); one GPU.

    The conditioning variants are scanned at thresholds 0 / 0 / 1; each must be valid with mac > 0.  Binary traits:
    ``Phi`` is scaled by the SPA factors ``d_j`` of ``seqAssocGLMM_spaSKAT`` (scanned rows and conditioning variants
    alike), so that without a correlated conditioning variant the conditional p-value of a row is its SPA p-value.
    Result: the columns of ``seqAssocGLMM_SPA``, then ``beta.cond``, ``SE.cond``, ``pval.cond`` (``cond_tests``;
    ``beta.cond`` refers to the alt allele like ``beta``).  A variant of the set itself, or one the set explains,
    gets NaN there.  ``res_savefn``: ``.rds`` / ``.RData``; the ``.gds`` writer has fixed columns and is refused.

    ``grm_mat`` (what ``seqAssocGLMM_spaSKAT(grm_mat=)`` accepts; every sample of the model must be in it) replaces
    ``Phi`` by the covariance under the fitted model itself, ``Phi^K = A' P A`` with ``Sigma = tau[0] diag(1/V) + tau[1] K``
    (``sgx_cond_kmat_set`` / ``sgx_cond_kmat_2bit``; solves to ``tol_pcg`` in at most ``maxiter_pcg`` steps):
    ``var_ratio`` does not enter it, the SPA scale factors are formed against ``Phi^K_jj``, ``cond_tests`` is the same
    code, and a column ``n.iter`` holds the PCG steps of the row's column.  Dosage input takes
    ``sgx_ds_block_cond_kmat_set`` / ``sgx_ds_block_cond_kmat`` on the resident rows.  Refused before any
    row is read: dosage input on a scanner without ``dosage_block`` or whose block has no ``cond_kmat``
    (``NotImplementedError``), a sample of the model missing from ``grm_mat`` (``ValueError``), a LOCO model."""
    check_scan_args(maf, mac, missing, spa_pval, var_ratio, dsnode, res_savefn, res_compress)
    if re.search(r"\.gds$", res_savefn, re.I):
        raise ValueError("The gds output has no columns for the conditional test; save to RData or RDS.")
    try:
        cond_ids = list(np.asarray(condition).ravel().tolist())
    except Exception:
        raise ValueError("`condition` should be a list of variant ids.") from None
    if not 1 <= len(cond_ids) <= COND_MAX:
        raise ValueError(f"`condition` should hold 1 to {COND_MAX} variant ids.")
    if len(set(cond_ids)) != len(cond_ids):
        raise ValueError("`condition` holds a variant id more than once.")
    if verbose:
        print("SAIGE conditional association analysis:")
    mod: NullModel = load_modobj(modobj, verbose)
    no_loco(mod, "seqAssocGLMM_SPA_cond")
    src = _open_source(gdsfile, verbose)
    in_mem = isinstance(src, GenotypeSource)
    if dsnode != "" and in_mem and src.packed is not None:
        raise NotImplementedError(_NO_DOSAGE)
    vid = np.asarray(src.variant_id if in_mem else src.read("variant.id"))
    where = {v: i for i, v in enumerate(vid.tolist())}
    unknown = [v for v in cond_ids if v not in where]
    if unknown:
        raise ValueError(f"`condition`: no variant with id {unknown[0]!r}.")
    cidx = [where[v] for v in cond_ids]

    inp = open_scan_input(src, mod, dsnode, verbose)
    if dsnode != "" and inp.kind == "packed":
        src.node(dsnode + "/data")      # a named node is a dosage node here: "$dosage_alt" is refused as the missing node it is
    kmat_w = None
    if grm_mat is not None:
        # dosage input needs a scanner with dosage blocks: a factory that is a class without them is refused unmade
        if inp.kind != "packed" and isinstance(scanner_factory, type) and not hasattr(scanner_factory, "dosage_block"):
            raise NotImplementedError(_NO_DOSAGE_KMAT)
        kmat_w = aligned_grm_mat(grm_mat, inp, mod)
    n_samp, n_var = inp.n_samp, inp.n_var
    if n_samp <= 0:
        raise ValueError("No sample in the genotypic data set!")
    if n_var <= 0:
        raise ValueError("No variant in the genotypic data set!")
    if not math.isfinite(var_ratio):
        var_ratio = float(np.nanmean(mod.var_ratio))
    if verbose:
        print(f"    # of samples: {_pretty(n_samp)}")
        print(f"    # of variants: {_pretty(n_var)}")
        print(f"    # of conditioning variants: {len(cidx)}")

    mobj = init_nullmod(mod, inp.ii, maf, mac, missing, spa_pval, var_ratio)
    if mod.trait_type not in ("binary", "quantitative"):
        raise ModelError("Invalid 'modobj$trait.type'.")
    binary = mod.trait_type == "binary"
    stored = inp.stored_ok(scanner_factory)
    if scanner_factory is None:
        from ._lib import Scanner
        require_device("seqAssocGLMM_SPA_cond")
        scanner_factory = Scanner
    sc = scanner_factory(mobj)
    try:
        thresholds = (float(maf), float(mac), float(missing), float(spa_pval))
        kmat = None if kmat_w is None else KmatSolve(*kmat_w, np.asarray(mobj.tau, dtype=np.float64), int(maxiter_pcg),
                                                     float(tol_pcg))
        if inp.kind != "packed":
            scan = _scan_dosage(sc, inp, stored, cidx, cond_ids, thresholds, kmat)
        elif kmat is None:
            scan = _scan_hard(sc, inp, cidx, cond_ids, thresholds)
        else:
            scan = _scan_kmat(sc, inp, cidx, cond_ids, thresholds, kmat)
    finally:
        sc.close()

    res, out_c, S_C, Phi_CC, n_iter = scan
    x = res[:, 8] != 0
    if verbose:
        print(f"# of variants after filtering by MAF, MAC and missing thresholds: {_pretty(int(x.sum()))}")
    ans = assemble_result(src, x, res[:, :8], mod.trait_type)
    o, S, var, cov = res[x, :8], res[x, 9], res[x, 10], res[x, 11:]
    d = d_C = None
    if binary:
        d = spa_scale(o, S, var, float(spa_pval))
        d_C = spa_scale(out_c, S_C, np.diag(Phi_CC), float(spa_pval))
    beta, se, p = cond_tests(S, var, cov, S_C, Phi_CC, d, d_C)
    ans["beta.cond"] = np.where(o[:, 0] > 0.5, -beta, beta)        # S is the flipped row's: back to the alt allele
    ans["SE.cond"], ans["pval.cond"] = se, p
    if n_iter is not None:
        ans["n.iter"] = n_iter[x]
    return finish_result(ans, res_savefn, res_compress, verbose, inp.sample_id() if res_savefn else None)
