"""The explicit GRM: ``seqFitDenseGRM`` and ``seqFitSparseGRM`` (SAIGE's ``createSparseGRM``, upstream SAIGEgds
2.x).

The reference this project follows (v1.12.5) has the GRM as an operator only, so the two GRM functions are
unpinned by it: they are tied to the pinned operator by identities (diagonal, K b = crossprod(b)) and to a
long-double reference (tests/grm_dense_ref.py).  K = G'G/M over the markers the null-model fit
would pick with the same arguments; the numbers come from ``sgx_grm_dense`` / ``sgx_grm_sparse``.
"""
from __future__ import annotations

import gzip
import re
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

DENSE_BUDGET_BYTES = 8 << 30      # seqFitDenseGRM refuses a matrix (8 N^2 bytes) above this: N <= 32768


@dataclass
class SparseGRM:
    """Upper triangle (i <= j, 0-based, sorted by (i, j)) of the thresholded GRM: every pair with
    K_ij >= rel_cutoff and every diagonal entry."""
    sample_id: List[str]
    n: int
    n_markers: int
    rel_cutoff: float
    i: np.ndarray
    j: np.ndarray
    x: np.ndarray

    def to_dense(self) -> np.ndarray:
        K = np.zeros((self.n, self.n), dtype=np.float64)
        K[self.i, self.j] = self.x
        K[self.j, self.i] = self.x
        return K

    def matvec(self, b) -> np.ndarray:
        """K b of the symmetric matrix, in double."""
        b = np.asarray(b, dtype=np.float64)
        if b.shape != (self.n,):
            raise ValueError("b must have one entry per sample")
        out = np.zeros(self.n, dtype=np.float64)
        np.add.at(out, self.i, self.x * b[self.j])
        off = self.i != self.j
        np.add.at(out, self.j[off], self.x[off] * b[self.i[off]])
        return out

    def subset(self, sample_id: Sequence[str]) -> "SparseGRM":
        """The matrix of those samples in that order: re-indexed, the entries of other samples dropped, i <= j,
        sorted by (i, j)."""
        ids = [str(s) for s in sample_id]
        if len(set(ids)) != len(ids):
            raise ValueError("'sample_id' should be unique.")
        pos = {s: k for k, s in enumerate(self.sample_id)}
        miss = [s for s in ids if s not in pos]
        if miss:
            raise ValueError(f"{len(miss)} sample(s) not in the GRM: {miss[:5]}")
        new = np.full(self.n, -1, dtype=np.int64)          # old index -> new index, -1: dropped
        new[[pos[s] for s in ids]] = np.arange(len(ids))
        a, b = new[self.i], new[self.j]
        keep = (a >= 0) & (b >= 0)
        a, b, x = a[keep], b[keep], self.x[keep]
        i, j = np.minimum(a, b), np.maximum(a, b)
        o = np.lexsort((j, i))
        return SparseGRM(sample_id=ids, n=len(ids), n_markers=self.n_markers, rel_cutoff=self.rel_cutoff,
                         i=i[o].astype(np.int32), j=j[o].astype(np.int32), x=np.ascontiguousarray(x[o]))

    def related_pairs(self) -> List[Tuple[str, str, float]]:
        """The off-diagonal entries as (sample id, sample id, kinship coefficient K_ij)."""
        off = np.flatnonzero(self.i != self.j)
        return [(self.sample_id[int(self.i[k])], self.sample_id[int(self.j[k])], float(self.x[k])) for k in off]


def _grm_inputs(gdsfile, sample_id, variant_id, maf, missing_rate, max_num_snp, seed, verbose, operator_factory):
    """Samples (file order, and the permutation to the caller's order) and markers as the null-model fit picks
    them, and the operator on them -> (sample ids in the caller's order, perm or None, op, n_markers, idx)."""
    from .assoc import _open_source
    from .fitnull import _select_grm_markers
    src = _open_source(gdsfile, verbose)
    gsid = [str(s) for s in src.sample_id()]
    perm = None
    if sample_id is None:
        sel, ids = list(range(len(gsid))), gsid
    else:
        ids = [str(s) for s in sample_id]
        if len(set(ids)) != len(ids):
            raise ValueError("'sample_id' should be unique.")
        pos = {s: k for k, s in enumerate(gsid)}
        miss = [s for s in ids if s not in pos]
        if miss:
            raise ValueError(f"'sample_id' not in the GDS file: {miss[:5]}")
        fidx = np.array([pos[s] for s in ids], dtype=np.int64)
        order = np.argsort(fidx, kind="stable")
        sel = [int(v) for v in fidx[order]]
        if not np.array_equal(order, np.arange(len(ids))):
            perm = np.empty(len(ids), dtype=np.int64)      # perm[k]: position in the file-ordered GRM of ids[k]
            perm[order] = np.arange(len(ids))
    if not sel:
        raise ValueError("No sample selected.")
    if verbose and variant_id is None:
        print("Selecting the GRM markers:")
    m = _select_grm_markers(src, sel, gsid, maf, missing_rate, max_num_snp, variant_id, seed, verbose,
                            use_gpu_counts=operator_factory is None)
    packed, idx = m["packed"], m["idx"]
    if idx.size == 0:
        raise ValueError("No marker passes the filter.")
    if verbose:
        print(f"    # of samples: {len(sel):,}")
        print(f"    # of variants: {idx.size:,}" + (f" (randomly selected from {m['n_before']:,})"
                                                     if m["n_before"] > idx.size else ""))
    if operator_factory is None:
        from ._lib import GrmOperator
        op = GrmOperator(packed, len(sel))
    else:
        op = operator_factory(packed, len(sel))
    return ids, perm, op, int(idx.size), np.asarray(m["var_ids"])[idx]


def _close(op):
    if hasattr(op, "close"):
        op.close()


def _save_rds_list(items, fn: str):
    from .results import _HEADER, _rlist
    with open(fn, "wb") as f:
        f.write(gzip.compress(_HEADER + _rlist(items)))


def seqFitDenseGRM(gdsfile, sample_id: Optional[Sequence[str]] = None, variant_id=None, maf: float = 0.005,
                   missing_rate: float = 0.01, max_num_snp: int = 1000000, seed: int = 200, out_fn: str = "",
                   verbose: bool = True, operator_factory=None):
    """The dense GRM of the markers the null-model fit picks -> (sample_id, K [N, N] float64).  ``sample_id=None``:
    all samples of the file in file order; else that subset in that order.  N is limited by
    ``DENSE_BUDGET_BYTES`` (8 N^2 bytes); beyond it use ``seqFitSparseGRM``.  ``out_fn``: ``.rds`` (an R list of
    ``sample.id`` and the matrix) or ``.npz``.  ``operator_factory(packed, n_samp)`` as in ``seqFitNullGLMM_SPA``:
    an object with ``dense()``."""
    from .assoc import _open_source
    src = _open_source(gdsfile, False)
    if sample_id is not None:
        sample_id = list(sample_id)
    n = len(src.sample_id()) if sample_id is None else len(sample_id)
    if 8 * n * n > DENSE_BUDGET_BYTES:
        raise ValueError(f"The dense GRM of {n:,} samples needs {8 * n * n / 2 ** 30:.1f} GiB, above the limit of "
                         f"{DENSE_BUDGET_BYTES / 2 ** 30:.0f} GiB: use seqFitSparseGRM, the thresholded sparse form.")
    _check_out_fn(out_fn)
    ids, perm, op, _, _ = _grm_inputs(src, sample_id, variant_id, maf, missing_rate, max_num_snp, seed, verbose,
                                      operator_factory)
    try:
        K = op.dense()
    finally:
        _close(op)
    if perm is not None:
        K = np.ascontiguousarray(K[np.ix_(perm, perm)])
    if out_fn:
        if re.search(r"\.npz$", out_fn, re.I):
            np.savez(out_fn, sample_id=np.asarray(ids), K=K)
        else:
            from .results import _num, _vector
            _save_rds_list([("sample.id", _vector(list(ids))), ("grm", _num(K))], out_fn)
    return ids, K


def seqFitSparseGRM(gdsfile, sample_id: Optional[Sequence[str]] = None, variant_id=None, maf: float = 0.005,
                    missing_rate: float = 0.01, max_num_snp: int = 1000000, rel_cutoff: float = 0.125, seed: int = 200,
                    out_fn: str = "", verbose: bool = True, operator_factory=None) -> SparseGRM:
    """The sparse GRM: the pairs with K_ij >= rel_cutoff and the diagonal, over the markers the null-model fit
    picks.  Arguments as ``seqFitDenseGRM``; the operator needs ``sparse(cutoff)``.  ``out_fn``: ``.rds`` (an R
    list of ``sample.id``, ``i``, ``j`` (1-based), ``x``, ``n``, ``rel.cutoff``) or ``.npz`` (the same arrays)."""
    if not np.isfinite(rel_cutoff):
        raise ValueError("'rel_cutoff' should be a finite number.")
    _check_out_fn(out_fn)
    ids, perm, op, n_markers, _ = _grm_inputs(gdsfile, sample_id, variant_id, maf, missing_rate, max_num_snp, seed,
                                              verbose, operator_factory)
    try:
        i, j, x = op.sparse(float(rel_cutoff))[:3]
    finally:
        _close(op)
    i, j, x = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(x, dtype=np.float64)
    if perm is not None:
        inv = np.empty_like(perm)                          # file-ordered position -> the caller's position
        inv[perm] = np.arange(perm.size)
        a, b = inv[i], inv[j]
        i, j = np.minimum(a, b), np.maximum(a, b)
        o = np.lexsort((j, i))
        i, j, x = i[o], j[o], x[o]
    res = SparseGRM(sample_id=list(ids), n=len(ids), n_markers=n_markers, rel_cutoff=float(rel_cutoff),
                    i=i.astype(np.int32), j=j.astype(np.int32), x=x)
    if verbose:
        print(f"    # of related pairs (>= {rel_cutoff:g}): {int((res.i != res.j).sum()):,}")
    if out_fn:
        if re.search(r"\.npz$", out_fn, re.I):
            np.savez(out_fn, sample_id=np.asarray(res.sample_id), i=res.i + 1, j=res.j + 1, x=res.x, n=res.n,
                     rel_cutoff=res.rel_cutoff)
        else:
            from .results import _vector
            _save_rds_list([("sample.id", _vector(list(res.sample_id))), ("i", _vector(res.i + 1)),
                            ("j", _vector(res.j + 1)), ("x", _vector(res.x)),
                            ("n", _vector(np.array([res.n], dtype=np.int32))),
                            ("rel.cutoff", _vector(np.array([res.rel_cutoff])))], out_fn)
    return res


def load_grm(fn: str):
    """Read what ``seqFitSparseGRM`` / ``seqFitDenseGRM`` wrote with ``out_fn`` (``.rds`` or ``.npz``): a
    ``SparseGRM`` (the files' 1-based i / j back to 0-based; they do not hold the marker count, so ``n_markers``
    is 0), or ``(sample_id, K)`` for a dense matrix."""
    _check_out_fn(fn)
    if re.search(r"\.npz$", fn, re.I):
        with np.load(fn) as z:
            d = {k: z[k] for k in z.files}
        d = {{"sample_id": "sample.id", "K": "grm", "rel_cutoff": "rel.cutoff"}.get(k, k): v for k, v in d.items()}
    else:
        from .rds import read_rds
        r = read_rds(fn)
        if not hasattr(r, "names") or "sample.id" not in r.names:
            raise ValueError(f"'{fn}' is not a GRM file of seqFitSparseGRM / seqFitDenseGRM.")
        d = {k: r[k] for k in r.names}
    ids = [str(s) for s in d["sample.id"]]
    if "grm" in d:
        K = np.ascontiguousarray(np.asarray(d["grm"], dtype=np.float64))
        if K.shape != (len(ids), len(ids)):
            raise ValueError(f"'{fn}': the matrix is {K.shape}, with {len(ids)} sample ids.")
        return ids, K
    if not all(k in d for k in ("i", "j", "x", "n", "rel.cutoff")):
        raise ValueError(f"'{fn}' is not a GRM file of seqFitSparseGRM / seqFitDenseGRM.")
    n = int(np.asarray(d["n"]).reshape(-1)[0])
    i, j = np.asarray(d["i"], dtype=np.int64) - 1, np.asarray(d["j"], dtype=np.int64) - 1
    x = np.ascontiguousarray(np.asarray(d["x"], dtype=np.float64))
    if n != len(ids) or i.shape != x.shape or j.shape != x.shape or (x.size and (i.min() < 0 or j.max() >= n or (i > j).any())):
        raise ValueError(f"'{fn}': inconsistent sparse GRM.")
    return SparseGRM(sample_id=ids, n=n, n_markers=0, rel_cutoff=float(np.asarray(d["rel.cutoff"]).reshape(-1)[0]),
                     i=i.astype(np.int32), j=j.astype(np.int32), x=x)


def _align_grm_mat(grm_mat, sample_id: Sequence[str]):
    """``grm_mat`` of ``seqFitNullGLMM_SPA`` (a ``SparseGRM``, ``(sample_id, K)`` or a file of ``load_grm``) as the
    matrix of the model's samples in their order: a ``SparseGRM`` or a square float64 array."""
    if isinstance(grm_mat, str):
        grm_mat = load_grm(grm_mat)
    ids = [str(s) for s in sample_id]

    def missing(have):
        have = set(have)
        miss = [s for s in ids if s not in have]
        if miss:
            raise ValueError(f"{len(miss)} sample(s) of the model are not in 'grm_mat': {miss[:5]}")

    if isinstance(grm_mat, SparseGRM):
        missing(grm_mat.sample_id)
        return grm_mat.subset(ids)
    try:
        gids, K = grm_mat
    except (TypeError, ValueError):
        raise ValueError("'grm_mat' should be a SparseGRM, (sample_id, K) or a file name.") from None
    gids = [str(s) for s in gids]
    K = np.asarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1] or K.shape[0] != len(gids):
        raise ValueError(f"'grm_mat' should be a square matrix with one row per sample id: it is "
                         f"{'x'.join(str(v) for v in K.shape)} with {len(gids)} sample ids.")
    if len(set(gids)) != len(gids):
        raise ValueError("The sample ids of 'grm_mat' should be unique.")
    missing(gids)
    if gids == ids:
        return np.ascontiguousarray(K)
    pos = {s: k for k, s in enumerate(gids)}
    ix = np.array([pos[s] for s in ids], dtype=np.int64)
    return np.ascontiguousarray(K[np.ix_(ix, ix)])


def _check_out_fn(out_fn: str):
    if out_fn and not re.search(r"\.(rds|npz)$", out_fn, re.I):
        raise ValueError("Unknown format of the output file, and it should be RDS or npz.")
