"""seqFitPCA -- the top principal components of the GRM, the ancestry covariates of the null model's ``formula``, and
``pca_project`` for the samples a decomposition left out.  The reference (v1.12.5) sends the user to SNPRelate's
``snpgdsPCA`` for them, which forms the dense N x N matrix; here the eigenpairs come from the operator the fit uses
(``sgx_grm_pca``: block subspace iteration around ``sgx_grm_crossprod_multi_dev``), so nothing N x N exists.
The algorithm, the summation orders and what is bit-stable: DESIGN.md 8o.
"""
from __future__ import annotations

import re
import warnings
from typing import Optional, Sequence

import numpy as np

from ._lib import PcaRankError  # noqa: F401  (an injected operator raises it; _lib.SgxRankError is one)
from .grm import _check_out_fn, _close, _grm_inputs, _save_rds_list

MAX_BLOCK = 64                # SGX_GRM_MAX_RHS: vectors of the iteration's block
_PROJECT_BYTES = 256 << 20    # pca_project: bytes of one float64 [rows, n] temporary of a pass (it holds a few of them)


def seqFitPCA(gdsfile, sample_id: Optional[Sequence[str]] = None, variant_id=None, n_pc: int = 20, n_extra: int = 12,
              maf: float = 0.005, missing_rate: float = 0.01, max_num_snp: int = 1000000, seed: int = 200,
              tol: float = 1e-6, max_iter: int = 100, snp_loading: bool = False, out_fn: str = "", verbose: bool = True,
              operator_factory=None) -> dict:
    """The top ``n_pc`` principal components of K = G'G/M over the markers the null-model fit picks with the same
    arguments (``variant_id``: those of ``seqFitLDpruning``, say) -> a dict with SNPRelate's names: ``sample.id``,
    ``snp.id``, ``eigenval`` [n_pc], ``eigenvect`` [N, n_pc] (the caller's sample order; unit columns, the entry of
    largest magnitude positive), ``varprop`` (eigenval / trace K), ``TraceXTX`` (trace K), ``resid`` (|K u - theta u|),
    ``converged`` (resid <= tol * eigenval[0], per component), ``n.iter``; with ``snp_loading`` also ``snploading``
    [n_pc, M], ``avgfreq`` and ``scale`` (the marker table), which ``pca_project`` needs.

    The iteration works on ``n_pc + n_extra`` vectors (at most 64, N and M) started from
    ``default_rng(seed).standard_normal``; the extra vectors buy the convergence rate
    (lambda_{n_pc + n_extra + 1} / lambda_{n_pc}) per round.  Components that did not meet ``tol`` within ``max_iter``
    give a warning, not an error.  ``out_fn``: ``.rds`` (an R list of those names) or ``.npz``.
    ``operator_factory(packed, n_samp)``: an object with ``pca(n_pc, Q0, max_iter, tol, loadings)``, ``diag()``,
    ``marker_table()`` and ``close()``."""
    _check_out_fn(out_fn)
    n_pc, n_extra = int(n_pc), int(n_extra)
    if n_pc < 1 or n_extra < 0:
        raise ValueError("'n_pc' should be at least 1 and 'n_extra' at least 0.")
    if not (np.isfinite(tol) and tol >= 0) or int(max_iter) < 1:
        raise ValueError("'tol' should be a finite number >= 0 and 'max_iter' at least 1.")
    ids, perm, op, n_markers, snp_id = _grm_inputs(gdsfile, sample_id, variant_id, maf, missing_rate, max_num_snp, seed,
                                                   verbose, operator_factory)
    try:
        n = len(ids)
        L = min(n_pc + n_extra, MAX_BLOCK, n, n_markers)
        if n_pc > L:
            raise ValueError(f"'n_pc' = {n_pc} is more than {L}: at most min(64, # of samples, # of markers) components.")
        Q0 = np.random.default_rng(seed).standard_normal((L, n))
        if verbose:
            print(f"Principal components: {n_pc} of a block of {L} vectors, tol {tol:g}, at most {int(max_iter)} rounds")
        try:
            r = op.pca(n_pc, Q0, max_iter=int(max_iter), tol=float(tol), loadings=bool(snp_loading))
        except PcaRankError:
            raise ValueError(f"The markers span fewer directions than n_pc + n_extra = {n_pc + n_extra} (the block of "
                             f"{L} vectors lost rank): lower 'n_extra' or 'n_pc', or use more markers.") from None
        trace = float(np.asarray(op.diag(), dtype=np.float64).sum())
        table = op.marker_table() if snp_loading else None
    finally:
        _close(op)
    eigval = np.asarray(r["eigval"], dtype=np.float64)
    resid = np.asarray(r["resid"], dtype=np.float64)
    vect = np.asarray(r["vec"], dtype=np.float64).T                 # [N, n_pc], file order
    if perm is not None:
        vect = vect[perm]
    converged = resid <= tol * eigval[0]
    res = {"sample.id": list(ids), "snp.id": np.asarray(snp_id), "eigenval": eigval,
           "eigenvect": np.ascontiguousarray(vect), "varprop": eigval / trace, "TraceXTX": trace, "resid": resid,
           "converged": converged, "n.iter": int(r["iters"])}
    if snp_loading:
        res["snploading"] = np.asarray(r["loading"], dtype=np.float64)
        res["avgfreq"], res["scale"] = (np.asarray(a, dtype=np.float64) for a in table)
    if verbose:
        print(f"    {int(converged.sum())} of {n_pc} converged in {res['n.iter']} round(s); "
              f"largest eigenvalue {eigval[0]:.6g} ({100 * res['varprop'][0]:.3g} % of the trace)")
    if not converged.all():
        warnings.warn(f"seqFitPCA: {int((~converged).sum())} of {n_pc} components did not reach tol = {tol:g} within "
                      f"{int(max_iter)} rounds (largest residual {resid.max():.3g}, eigenvalue {eigval[0]:.3g}).")
    if out_fn:
        _save_pca(res, out_fn)
    return res


_ARRAYS = ("eigenval", "eigenvect", "varprop", "resid", "snploading", "avgfreq", "scale")


def _save_pca(res: dict, out_fn: str):
    if re.search(r"\.npz$", out_fn, re.I):
        np.savez(out_fn, **{k.replace(".", "_"): np.asarray(v) for k, v in res.items()})
        return
    from .results import _num, _vector
    items = [("sample.id", _vector(list(res["sample.id"]))), ("snp.id", _vector(np.asarray(res["snp.id"])))]
    items += [(k, _num(res[k])) for k in _ARRAYS[:4]]
    items += [("TraceXTX", _vector(np.array([res["TraceXTX"]]))), ("converged", _vector(np.asarray(res["converged"]))),
              ("n.iter", _vector(np.array([res["n.iter"]], dtype=np.int32)))]
    items += [(k, _num(res[k])) for k in _ARRAYS[4:] if k in res]
    _save_rds_list(items, out_fn)


def load_pca(fn: str) -> dict:
    """Read what ``seqFitPCA`` wrote with ``out_fn`` (``.rds`` or ``.npz``) back into its dict."""
    _check_out_fn(fn)
    if re.search(r"\.npz$", fn, re.I):
        with np.load(fn) as z:
            d = {{"sample_id": "sample.id", "snp_id": "snp.id", "n_iter": "n.iter"}.get(k, k): z[k] for k in z.files}
    else:
        from .rds import read_rds
        r = read_rds(fn)
        if not hasattr(r, "names") or "eigenvect" not in r.names:
            raise ValueError(f"'{fn}' is not a file of seqFitPCA.")
        d = {k: r[k] for k in r.names}
    if "eigenvect" not in d or "sample.id" not in d:
        raise ValueError(f"'{fn}' is not a file of seqFitPCA.")
    out = {"sample.id": [str(s) for s in d["sample.id"]], "snp.id": np.asarray(d["snp.id"]),
           "TraceXTX": float(np.asarray(d["TraceXTX"]).reshape(-1)[0]),
           "converged": np.asarray(d["converged"]).astype(bool).reshape(-1),
           "n.iter": int(np.asarray(d["n.iter"]).reshape(-1)[0])}
    for k in _ARRAYS:
        if k in d:
            out[k] = np.ascontiguousarray(np.asarray(d[k], dtype=np.float64))
    return out


def _code_rows(src, rows: np.ndarray, sel: np.ndarray, n_all: int) -> np.ndarray:
    """The 2-bit codes [len(rows), len(sel)] of the file's rows ``rows`` (ascending) for the samples ``sel``."""
    from .assoc import GenotypeSource
    from .gds import round_dosage_codes, unpack_dosage_2bit
    if isinstance(src, GenotypeSource):
        if src.packed is not None:
            return unpack_dosage_2bit(np.asarray(src.packed)[rows], n_all)[:, sel]
        return round_dosage_codes(np.asarray(src.dosage)[rows][:, sel])
    out = np.empty((rows.size, sel.size), dtype=np.uint8)
    brk = np.flatnonzero(np.diff(rows) != 1) + 1                    # runs of consecutive rows: one read each
    for a, b in zip(np.concatenate([[0], brk]), np.concatenate([brk, [rows.size]])):
        v0, v1 = int(rows[a]), int(rows[b - 1]) + 1
        if src.has_genotype():
            out[a:b] = unpack_dosage_2bit(src.dosage_alt_packed_range(v0, v1, sample_sel=sel), sel.size)
        else:
            out[a:b] = round_dosage_codes(src.dosage_real_range("annotation/format/DS", v0, v1)[:, sel])
    return out


def pca_project(pca: dict, gdsfile, sample_id: Optional[Sequence[str]] = None, verbose: bool = True):
    """Scores of the samples of ``gdsfile`` (all, or ``sample_id`` in that order) on the components of a ``seqFitPCA``
    result made with ``snp_loading=True`` -> (sample ids, scores [n, n_pc]):
    score_ic = sum_v z_vi snploading[c, v] / sqrt(M eigenval_c), z the genotypes of ``pca["snp.id"]`` standardised
    with the stored ``avgfreq`` / ``scale`` and 0 where missing.  For a training sample that is its ``eigenvect``
    entry.  Host numpy, in passes of marker rows sized so that a float64 [rows, n] temporary stays within
    ``_PROJECT_BYTES`` (at most 4 096 rows): bounded memory at any n."""
    from .assoc import GenotypeSource, _open_source
    if not all(k in pca for k in ("snploading", "avgfreq", "scale")):
        raise ValueError("pca_project needs a seqFitPCA result made with snp_loading=True.")
    src = _open_source(gdsfile, verbose)
    gsid = [str(s) for s in src.sample_id()]
    ids = gsid if sample_id is None else [str(s) for s in sample_id]
    pos = {s: k for k, s in enumerate(gsid)}
    miss = [s for s in ids if s not in pos]
    if miss:
        raise ValueError(f"'sample_id' not in the GDS file: {miss[:5]}")
    sel = np.array([pos[s] for s in ids], dtype=np.int64)
    var_ids = np.asarray(src.variant_id if isinstance(src, GenotypeSource) else src.read("variant.id"))
    snp_id = np.asarray(pca["snp.id"])
    order = np.argsort(var_ids, kind="stable")
    at = np.searchsorted(var_ids[order], snp_id)
    if snp_id.size == 0 or (at >= var_ids.size).any() or (var_ids[order][np.minimum(at, var_ids.size - 1)] != snp_id).any():
        raise ValueError("Some of pca['snp.id'] are not among the file's variants.")
    rows = order[at]                                                # file row of marker k
    by_row = np.argsort(rows, kind="stable")
    load_, af, inv = (np.asarray(pca[k], dtype=np.float64) for k in ("snploading", "avgfreq", "scale"))
    eigval = np.asarray(pca["eigenval"], dtype=np.float64)
    m = snp_id.size
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(eigval > 0, 1 / np.sqrt(m * eigval), 0.0)
    scores = np.zeros((sel.size, eigval.size), dtype=np.float64)
    step = int(max(1, min(4096, _PROJECT_BYTES // (8 * max(1, sel.size)))))   # rows a pass: a byte budget over n
    for p0 in range(0, m, step):
        k = by_row[p0:p0 + step]                                    # markers of this pass, ascending file rows
        codes = _code_rows(src, rows[k], sel, len(gsid))
        z = np.where(codes == 3, 0.0, (codes.astype(np.float64) - 2 * af[k, None]) * inv[k, None])
        scores += z.T @ load_[:, k].T
    return ids, scores * w[None, :]
