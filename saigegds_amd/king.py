"""seqFitKING -- KING-robust kinship of the samples of a file, and ``unrelated_set`` on its pairs.

The standardised GRM's ``K_ij >= 0.125`` is inflated within every population of a structured sample, so it cannot
choose the unrelated samples a PCA is computed on.  KING-robust (Manichaikul et al. 2010, the between-family form;
SNPRelate's ``snpgdsIBDKING(type="KING-robust")``, to which the reference v1.12.5 sends the user) needs no allele
frequency: five integer counts per pair over the markers both samples are called at, from ``sgx_grm_king_counts`` /
``sgx_grm_king_pairs`` on the handle of the GRM operator.  Definition, kernel and what is bit-stable: DESIGN.md 8p.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import grm as _grm
from ._lib import king_values
from .grm import SparseGRM, _check_out_fn, _close, _grm_inputs, _save_rds_list

KIN_CUTOFF = 2.0 ** -4.5      # KING's lower edge of the third degree
DEGREE_EDGES = (2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5, 2.0 ** -4.5)   # above: 0 duplicate/MZ, 1, 2, 3; else -1
DENSE_BLOCK = 2048            # rows / columns per king_counts call of the dense form
_DENSE_BYTES_PER_PAIR = 20    # kinship and IBS0 in float64, n_snp in int32


@dataclass
class KingResult:
    """KING-robust kinship.  Sparse form (``kin_cutoff`` a number): ``i``, ``j`` (0-based, i < j, sorted by (i, j)) and
    ``kinship``, ``IBS0``, ``n_snp`` (markers called in both) per pair with kinship >= kin_cutoff.  Dense form
    (``kin_cutoff`` None): ``kinship``, ``IBS0``, ``n_snp`` are [n, n] matrices (NaN where a sample has no heterozygote
    in common calls) and ``i``, ``j`` are empty."""
    sample_id: List[str]
    n: int
    n_markers: int
    kin_cutoff: Optional[float]
    i: np.ndarray
    j: np.ndarray
    kinship: np.ndarray
    IBS0: np.ndarray
    n_snp: np.ndarray

    @property
    def is_dense(self) -> bool:
        return np.ndim(self.kinship) == 2

    def pairs(self, kin_cutoff: Optional[float] = None):
        """(i, j, kinship, IBS0) of the pairs i < j with kinship >= kin_cutoff (default: the result's own cutoff, or
        2^-4.5 for the dense form), sorted by (i, j)."""
        if self.is_dense:
            cut = KIN_CUTOFF if kin_cutoff is None else float(kin_cutoff)
            i, j = np.triu_indices(self.n, 1)
            kin, ibs = self.kinship[i, j], self.IBS0[i, j]
        else:
            cut = kin_cutoff
            i, j, kin, ibs = self.i, self.j, self.kinship, self.IBS0
        if cut is not None:
            with np.errstate(invalid="ignore"):
                keep = kin >= cut
            i, j, kin, ibs = i[keep], j[keep], kin[keep], ibs[keep]
        return i.astype(np.int32), j.astype(np.int32), np.asarray(kin, dtype=np.float64), np.asarray(ibs, dtype=np.float64)

    def related_pairs(self, kin_cutoff: Optional[float] = None) -> List[Tuple[str, str, float, float]]:
        """The pairs as (sample id, sample id, kinship, IBS0)."""
        i, j, kin, ibs = self.pairs(kin_cutoff)
        return [(self.sample_id[int(a)], self.sample_id[int(b)], float(k), float(z)) for a, b, k, z in zip(i, j, kin, ibs)]

    def degree(self, kin_cutoff: Optional[float] = None) -> np.ndarray:
        """KING's inference band per pair of ``pairs()``: 0 duplicate / MZ twin (kinship > 2^-1.5), 1 first degree
        (> 2^-2.5), 2 second (> 2^-3.5), 3 third (> 2^-4.5), -1 below."""
        return degree_of(self.pairs(kin_cutoff)[2])

    def to_dense(self) -> np.ndarray:
        """Kinship as an [n, n] matrix, for small n: the listed pairs, 0.5 on the diagonal, 0 elsewhere (the dense
        form: its matrix)."""
        if self.is_dense:
            return np.array(self.kinship, dtype=np.float64)
        K = np.zeros((self.n, self.n), dtype=np.float64)
        K[self.i, self.j] = self.kinship
        K[self.j, self.i] = self.kinship
        np.fill_diagonal(K, 0.5)
        return K


def degree_of(kinship) -> np.ndarray:
    """KING's inference bands of kinship values (see ``KingResult.degree``); NaN gives -1."""
    k = np.asarray(kinship, dtype=np.float64)
    out = np.full(k.shape, -1, dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for d, edge in reversed(list(enumerate(DEGREE_EDGES))):
            out[k > edge] = d
    return out


def _dense_counts(op, n: int) -> np.ndarray:
    """int32 [5, n, n] from king_counts in blocks: those on and above the diagonal, the others mirrored with hi and hj
    swapped (counts (j, i) are counts (i, j) with the two swapped)."""
    c = np.empty((5, n, n), dtype=np.int32)
    for i0 in range(0, n, DENSE_BLOCK):
        ni = min(DENSE_BLOCK, n - i0)
        for j0 in range(i0, n, DENSE_BLOCK):
            nj = min(DENSE_BLOCK, n - j0)
            blk = np.asarray(op.king_counts(i0, ni, j0, nj))
            c[:, i0:i0 + ni, j0:j0 + nj] = blk
            if j0 != i0:
                c[:, j0:j0 + nj, i0:i0 + ni] = blk[[0, 2, 1, 3, 4]].transpose(0, 2, 1)
    return c


def seqFitKING(gdsfile, sample_id: Optional[Sequence[str]] = None, variant_id=None, maf: float = 0.005,
               missing_rate: float = 0.01, max_num_snp: int = 1000000, kin_cutoff: Optional[float] = KIN_CUTOFF,
               seed: int = 200, out_fn: str = "", verbose: bool = True, operator_factory=None) -> KingResult:
    """KING-robust kinship over the markers the null-model fit picks with the same arguments (``variant_id``: those of
    ``seqFitLDpruning``, say) -> ``KingResult``: every pair with kinship >= ``kin_cutoff`` (default 2^-4.5, third degree
    and closer), or with ``kin_cutoff=None`` the full kinship / IBS0 / n_snp matrices (SNPRelate's shape of result;
    limited by ``grm.DENSE_BUDGET_BYTES`` at 20 bytes a pair).  ``sample_id=None``: all samples in file order; else
    that subset in that order.  ``out_fn``: ``.rds`` or ``.npz``, read back by ``load_king``.
    ``operator_factory(packed, n_samp)``: an object with ``king_pairs(cutoff)`` and ``king_counts(i0, ni, j0, nj)``."""
    if kin_cutoff is not None and not np.isfinite(kin_cutoff):
        raise ValueError("'kin_cutoff' should be a finite number or None.")
    _check_out_fn(out_fn)
    if kin_cutoff is None:
        from .assoc import _open_source
        gdsfile = _open_source(gdsfile, False)
        n = len(gdsfile.sample_id()) if sample_id is None else len(list(sample_id))
        if _DENSE_BYTES_PER_PAIR * n * n > _grm.DENSE_BUDGET_BYTES:
            raise ValueError(f"The kinship matrices of {n:,} samples need {_DENSE_BYTES_PER_PAIR * n * n / 2 ** 30:.1f} "
                             f"GiB, above the limit of {_grm.DENSE_BUDGET_BYTES / 2 ** 30:.0f} GiB: give 'kin_cutoff' "
                             "for the list of related pairs.")
    if sample_id is not None:
        sample_id = list(sample_id)
    ids, perm, op, n_markers, _ = _grm_inputs(gdsfile, sample_id, variant_id, maf, missing_rate, max_num_snp, seed,
                                              verbose, operator_factory)
    n = len(ids)
    try:
        if kin_cutoff is None:
            counts = _dense_counts(op, n)
        else:
            i, j, kin, ibs, counts = op.king_pairs(float(kin_cutoff))[:5]
    finally:
        _close(op)
    if kin_cutoff is None:
        if perm is not None:                               # (hi and hj follow their samples: no swap)
            counts = np.ascontiguousarray(counts[:, perm][:, :, perm])
        kin, ibs = king_values(counts)
        res = KingResult(sample_id=list(ids), n=n, n_markers=n_markers, kin_cutoff=None, i=np.empty(0, dtype=np.int32),
                         j=np.empty(0, dtype=np.int32), kinship=kin, IBS0=ibs, n_snp=np.ascontiguousarray(counts[0]))
    else:
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        kin, ibs = np.asarray(kin, dtype=np.float64), np.asarray(ibs, dtype=np.float64)
        nn = np.asarray(counts, dtype=np.int32).reshape(-1, 5)[:, 0]
        if perm is not None:
            inv = np.empty_like(perm)                      # file-ordered position -> the caller's position
            inv[perm] = np.arange(perm.size)
            a, b = inv[i], inv[j]
            i, j = np.minimum(a, b), np.maximum(a, b)
            o = np.lexsort((j, i))
            i, j, kin, ibs, nn = i[o], j[o], kin[o], ibs[o], nn[o]
        res = KingResult(sample_id=list(ids), n=n, n_markers=n_markers, kin_cutoff=float(kin_cutoff),
                         i=i.astype(np.int32), j=j.astype(np.int32), kinship=np.ascontiguousarray(kin),
                         IBS0=np.ascontiguousarray(ibs), n_snp=np.ascontiguousarray(nn))
        if verbose:
            print(f"    # of related pairs (kinship >= {kin_cutoff:g}): {res.i.size:,}")
    if out_fn:
        _save_king(res, out_fn)
    return res


def _save_king(res: KingResult, out_fn: str):
    cut = np.array([np.nan if res.kin_cutoff is None else res.kin_cutoff])
    if re.search(r"\.npz$", out_fn, re.I):
        np.savez(out_fn, sample_id=np.asarray(res.sample_id), i=res.i + 1, j=res.j + 1, kinship=res.kinship, IBS0=res.IBS0,
                 n_snp=res.n_snp, n=res.n, n_markers=res.n_markers, kin_cutoff=cut)
        return
    from .results import _num, _vector
    _save_rds_list([("sample.id", _vector(list(res.sample_id))), ("i", _vector(res.i + 1)), ("j", _vector(res.j + 1)),
                    ("kinship", _num(res.kinship)), ("IBS0", _num(res.IBS0)), ("n.snp", _num(res.n_snp)),
                    ("n", _vector(np.array([res.n], dtype=np.int32))),
                    ("n.markers", _vector(np.array([res.n_markers], dtype=np.int32))), ("kin.cutoff", _vector(cut))],
                   out_fn)


def load_king(fn: str) -> KingResult:
    """Read what ``seqFitKING`` wrote with ``out_fn`` (``.rds`` or ``.npz``; the files' 1-based i / j back to 0-based)."""
    _check_out_fn(fn)
    names = {"sample_id": "sample.id", "n_snp": "n.snp", "n_markers": "n.markers", "kin_cutoff": "kin.cutoff"}
    if re.search(r"\.npz$", fn, re.I):
        with np.load(fn) as z:
            d = {names.get(k, k): z[k] for k in z.files}
    else:
        from .rds import read_rds
        r = read_rds(fn)
        if not hasattr(r, "names"):
            raise ValueError(f"'{fn}' is not a file of seqFitKING.")
        d = {k: r[k] for k in r.names}
    if not all(k in d for k in ("sample.id", "i", "j", "kinship", "IBS0", "n.snp", "n", "n.markers", "kin.cutoff")):
        raise ValueError(f"'{fn}' is not a file of seqFitKING.")
    ids = [str(s) for s in d["sample.id"]]
    n = int(np.asarray(d["n"]).reshape(-1)[0])
    cut = float(np.asarray(d["kin.cutoff"]).reshape(-1)[0])
    i, j = np.asarray(d["i"], dtype=np.int64).reshape(-1) - 1, np.asarray(d["j"], dtype=np.int64).reshape(-1) - 1
    kin, ibs = (np.ascontiguousarray(np.asarray(d[k], dtype=np.float64)) for k in ("kinship", "IBS0"))
    nn = np.ascontiguousarray(np.asarray(d["n.snp"]).astype(np.int32))
    dense = np.isnan(cut)
    shape = (n, n) if dense else i.shape
    if n != len(ids) or kin.shape != shape or ibs.shape != shape or nn.shape != shape or i.shape != j.shape or (
            i.size and (i.min() < 0 or j.max() >= n or (i >= j).any())):
        raise ValueError(f"'{fn}': inconsistent KING result.")
    return KingResult(sample_id=ids, n=n, n_markers=int(np.asarray(d["n.markers"]).reshape(-1)[0]),
                      kin_cutoff=None if dense else cut, i=i.astype(np.int32), j=j.astype(np.int32), kinship=kin, IBS0=ibs,
                      n_snp=nn)


def unrelated_set(pairs, sample_id: Optional[Sequence[str]] = None, kin_cutoff: Optional[float] = None):
    """A maximal set of mutually unrelated samples -> (unrelated ids, related ids), both in the order of the samples.

    ``pairs``: a ``KingResult`` (its pairs with kinship >= ``kin_cutoff``; default: all it lists, or 2^-4.5 for the
    dense form) or a ``SparseGRM`` (its off-diagonal entries >= ``kin_cutoff``; default: all).  ``sample_id``: restrict
    to those samples (pairs with any other sample are ignored).  Deterministic: while a related pair remains among the
    kept samples, the kept sample with the most remaining relatives is dropped -- ties: the larger sum of kinship to
    them, then the higher index, so earlier samples survive; then dropped samples are re-admitted in ascending index
    order where no relative of theirs is kept, so the set is maximal.  Host code."""
    if isinstance(pairs, KingResult):
        i, j, w, _ = pairs.pairs(kin_cutoff)
    elif isinstance(pairs, SparseGRM):
        off = pairs.i != pairs.j
        i, j, w = pairs.i[off], pairs.j[off], np.asarray(pairs.x, dtype=np.float64)[off]
        if kin_cutoff is not None:
            keep = w >= float(kin_cutoff)
            i, j, w = i[keep], j[keep], w[keep]
    else:
        raise ValueError("'pairs' should be a KingResult or a SparseGRM.")
    ids, n = list(pairs.sample_id), int(pairs.n)
    inside = np.ones(n, dtype=bool)
    if sample_id is not None:
        pos = {s: k for k, s in enumerate(ids)}
        want = [str(s) for s in sample_id]
        miss = [s for s in want if s not in pos]
        if miss:
            raise ValueError(f"{len(miss)} sample(s) not among the pairs' samples: {miss[:5]}")
        inside[:] = False
        inside[[pos[s] for s in want]] = True
    nbr = [dict() for _ in range(n)]                       # relatives of a sample among `inside`: index -> kinship
    for a, b, x in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), np.asarray(w).tolist()):
        if a != b and inside[a] and inside[b]:
            nbr[a][b] = x
            nbr[b][a] = x
    kept = inside.copy()
    deg = np.array([len(d) for d in nbr], dtype=np.int64)  # remaining relatives among the kept samples
    ksum = np.array([sum(d.values()) for d in nbr], dtype=np.float64)
    while True:
        cand = np.flatnonzero(kept & (deg > 0))
        if cand.size == 0:
            break
        top = cand[deg[cand] == deg[cand].max()]
        top = top[ksum[top] == ksum[top].max()]
        k = int(top.max())
        kept[k] = False
        deg[k] = 0
        for r in nbr[k]:
            if kept[r]:
                deg[r] -= 1
                ksum[r] = sum(x for q, x in nbr[r].items() if kept[q])   # over the kept relatives, afresh: no drift
    for k in np.flatnonzero(inside & ~kept).tolist():
        if not any(kept[r] for r in nbr[k]):
            kept[k] = True
    return ([ids[k] for k in np.flatnonzero(kept)], [ids[k] for k in np.flatnonzero(inside & ~kept)])
