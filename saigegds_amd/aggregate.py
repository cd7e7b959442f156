"""Aggregate tests on MI355X: burden, ACAT-V and ACAT-O.

Python mirror of ``seqAssocGLMM_spaBurden()``, ``seqAssocGLMM_spaACAT_V()``,
``seqAssocGLMM_spaACAT_O()`` and ``pACAT()`` (reference R/assoc_aggregate.r:51-797,
native side src/saige_main.cpp:466-1052).  The reference calls one native routine per
unit; here the units go through the scan library in batches.  One flow serves the three drivers and the SKAT driver
(``skat.py``): ``_prepare`` opens the input, the model (thresholds 0 / 0 / 1 as ``.init_nullmod(modobj, ii, 0, 0, 1,
...)`` sets them) and the scanner; ``_run`` then takes the batches of units of a rows backend, and per batch

1. loads the batch's distinct variants: counts and the single-variant scan table;
2. forms the per-variant maf and mac of ``ds_mat_mafmac`` and the single-variant p-values of ACAT-V
   (``variant_stats``);
3. for SKAT, selects each unit's variants and takes their score statistics and covariance (``skat_step``);
4. for the driver's burden columns, makes the normalised weights, the flip and the mean of ``ds_mat_burden``
   (``_burden_entries``) and has the device collapse the rows -- weighted, mean-imputed, minor-allele-oriented --
   and put them through the same single-variant test;

the Cauchy combination (``acat_pval``) follows on the host.  The two backends:

* 2-bit genotypes (``$dosage_alt``, the RAW branch of the reference routines; also an integer matrix that holds hard
  calls only, ``reduce_hard_calls``): ``_packed_rows``, one batch with every unit -- one ``sgx_scan_2bit``, one
  ``sgx_burden_2bit`` per column kind over all (unit, weight) rows, one ``sgx_skat_2bit``;
* dosages -- a format node such as ``annotation/format/DS``, or a ``GenotypeSource(dosage=...)`` of uint8, int32 or
  float64 (the INTSXP / REALSXP branches): ``_dosage_rows``, batches of consecutive units whose distinct variants fit
  a byte budget on the device; the rows of a batch are uploaded once to a ``DosageBlock`` and everything above is
  made from the resident rows.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import math
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ._lib import Scanner
from .assoc import PackedRows, ScanInput, _is_num, open_scan_input
from .gds import pack_dosage_2bit, unpack_dosage_2bit
from .kmat import NO_DOSAGE_KMAT
from .nullmod import NullModel, ScanModel, init_nullmod, load_modobj, no_loco

# AggrParamBeta, R/assoc_aggregate.r:18-19: columns (shape1, shape2) = (1,1) and (1,25)
AggrParamBeta = np.array([[1.0, 1.0], [1.0, 25.0]]).T     # [2, n_weights]

ROUND_ZERO = 1e-300
ROUND_ONE = 1 - 1e-16


def _dbeta(x: np.ndarray, a: float, b: float) -> np.ndarray:
    """``Rf_dbeta(x, a, b, FALSE)``."""
    from scipy.stats import beta
    return beta.pdf(np.asarray(x, dtype=np.float64), a, b)


def acat_pval(pval: Sequence[float], w: Optional[Sequence[float]] = None, throw_error: bool = False) -> float:
    """``acat_pval`` (src/saige_main.cpp:1001-1052)."""
    p = np.asarray(pval, dtype=np.float64)
    w = np.ones_like(p) if w is None else np.asarray(w, dtype=np.float64)
    ok = np.isfinite(p) & np.isfinite(w)
    sumw = float(np.sum(w[ok]))
    if sumw <= 0:
        if throw_error:
            raise ValueError("the sum of weights should be > 0.")
        return float("nan")
    tstat = 0.0
    for pi, wi in zip(p[ok], w[ok]):
        if pi < 0 or pi > 1:
            if throw_error:
                raise ValueError(f"Invalid input p-value: {pi:g}.")
            return float("nan")
        pi = ROUND_ZERO if pi < ROUND_ZERO else (ROUND_ONE if pi > ROUND_ONE else pi)
        if pi >= 1e-15:
            tstat += wi * math.tan(math.pi * (0.5 - pi))
        else:
            tstat += wi / pi / math.pi
    tstat /= sumw
    if tstat <= 5e14:
        return 0.5 - math.atan(tstat) / math.pi
    return 1.0 / tstat / math.pi


def pACAT(p: Sequence[float], w: Optional[Sequence[float]] = None) -> float:
    """``pACAT(p, w)`` (R/assoc_aggregate.r; native ``saige_acat_p``, :1054-1082)."""
    p = np.asarray(p, dtype=np.float64)
    if p.size <= 0:
        raise ValueError("the number of p-values should be > 0.")
    if p.size == 1:
        return float(p[0])
    if w is not None and len(w) != p.size:
        raise ValueError("weights should have the same length as p-values.")
    return acat_pval(p, w, throw_error=True)


def pACAT2(p: Sequence[float], maf: Sequence[float], wbeta=(1, 25)) -> float:
    """``pACAT2(p, maf, wbeta)`` (R/saige_main.r:150-156): ACAT with weights dbeta(maf)^2 maf (1 - maf)."""
    p, maf = np.asarray(p, dtype=np.float64), np.asarray(maf, dtype=np.float64)
    if len(wbeta) != 2:
        raise ValueError("length(wbeta) == 2L is not TRUE")
    if p.size != maf.size:
        raise ValueError("length(p) == length(maf) is not TRUE")
    w = _dbeta(maf, float(wbeta[0]), float(wbeta[1]))
    return pACAT(p, w * w * maf * (1 - maf))


def _mean_sd(x: np.ndarray):
    """``f64_mean_sd``: mean and sample sd over finite values."""
    x = x[np.isfinite(x)]
    if x.size == 0:
        return float("nan"), float("nan")
    return float(np.mean(x)), (float(np.std(x, ddof=1)) if x.size > 1 else float("nan"))


def _minmax(x: np.ndarray):
    x = x[np.isfinite(x)]
    if x.size == 0:
        return float("nan"), float("nan")
    return float(np.min(x)), float(np.max(x))


class _Units:
    """``SeqUnitListClass``: ``units$desp`` (columns) and ``units$index`` (1-based variant
    indices per unit).  Accepts a dict with keys 'desp'/'index' or a plain list of index lists."""

    def __init__(self, units):
        if isinstance(units, dict):
            self.desp = dict(units.get("desp", {}))
            self.index = [np.asarray(ix, dtype=np.int64) for ix in units["index"]]
        else:
            self.index = [np.asarray(ix, dtype=np.int64) for ix in units]
            self.desp = {}
        if not self.index:
            raise TypeError("inherits(units, \"SeqUnitListClass\") is not TRUE")


def _check_beta(wbeta) -> np.ndarray:
    """``.check_beta``: a length-two vector or a matrix with two rows -> [2, n_weights]."""
    wb = np.asarray(wbeta, dtype=np.float64)
    if not np.all(np.isfinite(wb)):
        raise TypeError("is.finite(wbeta) is not TRUE")
    if wb.ndim == 1:
        if wb.size != 2:
            raise ValueError("'wbeta' should be a length-two vector or a matrix with two rows.")
        wb = wb.reshape(2, 1)
    elif wb.ndim != 2 or wb.shape[0] != 2 or wb.shape[1] <= 0:
        raise ValueError("'wbeta' should be a length-two vector or a matrix with two rows.")
    return wb


@dataclasses.dataclass(slots=True)
class _Prepared:
    """A set-test driver's call: what ``_prepare`` opens and ``_run`` fills.  The per-variant arrays hold one row per
    distinct variant of the units, in ascending order of the variant index."""
    units: _Units
    wbeta: np.ndarray                       # [2, n_weights]
    inp: ScanInput = None                   # the opened input
    sm: ScanModel = None                    # the model at thresholds 0 / 0 / 1
    binary: bool = False
    wb_colnm: List[str] = None              # "b<a>_<b>" per weight set
    sc: Any = None                          # the scanner; the driver closes it
    backend: Any = None                     # the rows backend, not yet entered (_packed_rows / _dosage_rows)
    index: List[np.ndarray] = None          # per unit: rows of the per-variant arrays
    n: np.ndarray = None                    # per variant: non-missing samples,
    s: np.ndarray = None                    # their sum (a double sum for real dosages),
    maf: np.ndarray = None
    mac: np.ndarray = None
    pval: np.ndarray = None                 # the single-variant p-value (NaN: rejected by the scan's filter)
    out: np.ndarray = None                  # the scan table [n, 8] and
    valid: np.ndarray = None                # its valid flags
    burden: Dict[str, Any] = None           # column kind -> (burden rows [n_units, n_weights, 8], valid)
    skat: List[SkatStep] = None             # the SKAT driver: the device step of every batch of units
    collapse_mac: float = float("nan")      # SKAT / SKAT-O: variants up to this mac become one pseudo-variant a unit (NaN: off)
    n_collapsed: np.ndarray = None          # per unit: the variants its pseudo-variant replaces, and
    pseudo: np.ndarray = None               # its row of the per-variant arrays (appended to them; -1: none)


DS_BUDGET = 1 << 30      # bytes of dosage rows resident on the device per batch of units


def ds_row_bytes(dtype, n_samp: int) -> int:
    """Bytes of one resident dosage row: uint8 rows stay bytes, int32 and float64 rows are held as doubles."""
    return n_samp * (1 if np.dtype(dtype) == np.uint8 else 8)


def load_rows(blk, rows):
    """What a dosage reader returned -> the block: rows as the file stores them, or decoded rows."""
    return blk.load_packed(*rows.args()) if isinstance(rows, PackedRows) else blk.load(rows)


def flip_mean(n, s):
    """The scan's own imputation and flip of rows from their counts (n non-missing, s their double sum) ->
    (flip = s > n as uint8, mean = s / n, or 2 - s / n where flipped)."""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s / n
    fl = s > n
    return fl.astype(np.uint8), np.where(fl, 2 - m, m)


def dosage_tables(flip, mean, w=None) -> np.ndarray:
    """The value of each 2-bit code per row, [m, 4]: {0, 1, 2, mean} w, or {2, 1, 0, mean} w where ``flip`` -- ``mean``
    stands in for the missing code and is the flipped row's own (``flip_mean``: 2 - s / n there).  The one definition
    of these tables on the host; ``cond._tables`` restates it in torch for rows that stay on the device."""
    mean = np.asarray(mean, dtype=np.float64)
    w = np.ones_like(mean) if w is None else w
    t = np.stack([0 * w, w, 2 * w, mean * w], axis=1)
    return np.where(np.asarray(flip)[:, None] != 0, t[:, [2, 1, 0, 3]], t)


def reduce_hard_calls(inp: ScanInput) -> ScanInput:
    """An in-memory integer matrix that holds 0, 1, 2 and the missing code only has the meaning of the reference's RAW
    branch: the same input as 2-bit rows.  Any other input comes back as it is."""
    ds = inp.ds_all
    if inp.kind != "dosage" or not inp.in_mem or inp.ds_dtype == np.float64:
        return inp
    miss = 0xFF if ds.dtype == np.uint8 else np.iinfo(np.int32).min
    if not np.all((ds == miss) | ((ds >= 0) & (ds <= 2))):
        return inp
    codes = np.where((ds < 0) | (ds > 2), 3, ds).astype(np.uint8)
    return dataclasses.replace(inp, kind="packed", packed=pack_dosage_2bit(codes), ds_all=None, ds_dtype=None)


def variant_stats(n, s, out, valid):
    """``ds_mat_mafmac`` (src/saige_main.cpp:466-524) from a variant's counts (n non-missing, s their sum) and its row of
    the scan table -> (maf, mac, pval); ``single_test_*`` gives NaN where the scan's filter rejects."""
    with np.errstate(invalid="ignore", divide="ignore"):
        af = s / (2 * n)
    return np.where(n > 0, np.minimum(af, 1 - af), np.nan), np.minimum(s, 2 * n - s), np.where(valid != 0, out[:, 5], np.nan)


# ---- the rows backends: batches (of units), load, burden, skat ------------------------------------------------------
# load(bv): the distinct variants bv of a batch -> (n, s, st, out, valid): n non-missing, s their (double) sum, st the
#   truncated `int sum` of ds_mat_burden, and the scan table of the rows;
# burden(grp_ptr, var_idx, flip, mean, W): groups (CSR over rows of bv) x the columns of W ([entries, n_cols], NaN =
#   entry not in that column) -> (burden rows [groups * n_cols, 8] or [groups, n_cols, 8], valid);
# skat(unit_ptr, var_idx, flip, mean) -> (score [entries], cov per unit, PCG steps per entry or None);
# collapse(grp_ptr, var_idx, flip): groups (CSR over the resident rows) -> what load returns, for one pseudo-variant per
#   group; their rows are resident after the batch's own from then on.  None: the backend has none.

@contextlib.contextmanager
def _packed_rows(pr: _Prepared, used, kmat=None):
    """2-bit rows: one batch with every unit.  ``kmat`` (a ``KmatSolve``): SKAT's covariance on the explicit GRM
    (``sgx_skat_kmat_2bit``) instead of ``sgx_skat_2bit``."""
    sc, nw = pr.sc, pr.wbeta.shape[1]
    packed = pr.inp.packed_rows_at(used - 1)

    def scan(rows):
        out, valid = sc.scan_2bit(rows)
        ok = valid != 0
        n = np.where(ok, out[:, 2], 0).astype(np.float64)
        s = np.where(ok, np.rint(out[:, 0] * 2 * n), 0.0)           # RAW branch: s = sum of codes
        if not ok.all():    # a variant rejected by the scan's filter (monomorphic: maf = 0) still has counts: from the host
            codes = unpack_dosage_2bit(rows[~ok], pr.inp.n_samp).astype(np.int64)
            n[~ok], s[~ok] = (codes != 3).sum(axis=1), np.where(codes != 3, codes, 0).sum(axis=1)
        return n, s, s.astype(np.int64), out, valid                 # integer codes: nothing to truncate

    def load(bv):
        return scan(packed)

    def collapse(grp_ptr, var_idx, flip):
        nonlocal packed
        rows, _ = sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
        packed = np.concatenate([packed, rows])                     # burden and skat below read the longer matrix
        return scan(rows)

    def burden(grp_ptr, var_idx, flip, mean, W):
        ng = len(grp_ptr) - 1
        grp = np.repeat(np.arange(ng), np.diff(grp_ptr))
        res = []
        for c0 in range(0, W.shape[1], nw):       # one call per column kind, its rows ordered (unit, weight set)
            e, c = np.nonzero(np.isfinite(W[:, c0:c0 + nw]))
            row = grp[e] * nw + c
            o = np.argsort(row, kind="stable")
            e, c = e[o], c[o]
            row_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=ng * nw))])
            out, valid = sc.burden_2bit(packed, row_ptr, var_idx[e], dosage_tables(flip[e], mean[e], W[e, c0 + c]))
            res.append((out.reshape(ng, nw, 8), valid.reshape(ng, nw)))
        return np.concatenate([o for o, _ in res], axis=1), np.concatenate([v for _, v in res], axis=1)

    def skat(unit_ptr, var_idx, flip, mean):
        lut = dosage_tables(flip, mean)
        if kmat is None:
            return (*sc.skat_2bit(packed, unit_ptr, var_idx, lut), None)
        with kmat.operator(sc) as op:
            return sc.skat_kmat(op, packed, unit_ptr, var_idx, lut, *kmat.args)

    yield SimpleNamespace(batches=[list(range(len(pr.index)))], load=load, burden=burden, skat=skat,
                          collapse=collapse if hasattr(sc, "collapse_2bit") else None)


@contextlib.contextmanager
def _dosage_rows(pr: _Prepared, used, stored, budget, kmat=None):
    """Dosage rows: batches of consecutive units whose distinct variants fit ``budget`` bytes of resident rows (a unit
    larger than that is a batch of its own); one ``DosageBlock`` of the largest batch's size, one upload per batch.  A
    variant that two batches share (sliding windows) is loaded in both.  ``skat`` is None where the block has none.
    ``kmat`` (as for ``_packed_rows``): ``skat`` is the block's ``skat_kmat`` (``sgx_ds_block_skat_kmat``) on one operator
    for all batches; a scanner without ``dosage_block`` or a block without ``skat_kmat`` is refused before any row is
    read.  With pr.collapse_mac every unit of a batch counts one more resident row, its pseudo-variant, and the block has
    room for them after the batch's own rows (``collapse``: the block's, ``sgx_ds_block_collapse``); a block without
    ``collapse`` is refused before any row is read."""
    read_rows, dtype = pr.inp.dosage_reader(stored), pr.inp.ds_dtype
    row_bytes = ds_row_bytes(dtype, pr.sm.n)
    extra = 0 if math.isnan(pr.collapse_mac) else 1                # resident rows a unit adds of its own: its pseudo-variant
    batches, cur, seen = [], [], set()
    for u, r in enumerate(pr.index):
        new = set(r.tolist()) - seen
        if cur and (len(seen) + len(new) + extra * (len(cur) + 1)) * row_bytes > budget:
            batches.append(cur)
            cur, seen, new = [], set(), set(r.tolist())
        cur.append(u)
        seen |= new
    batches.append(cur)
    cap = max(np.unique(np.concatenate([pr.index[u] for u in bt])).size for bt in batches)
    cap += extra * max(len(bt) for bt in batches)
    if kmat is not None and not hasattr(pr.sc, "dosage_block"):
        raise NotImplementedError(NO_DOSAGE_KMAT.format("SKAT"))
    with contextlib.ExitStack() as stack:
        blk = stack.enter_context(pr.sc.dosage_block(dtype, cap))
        if extra and not hasattr(blk, "collapse"):
            raise NotImplementedError(NO_DOSAGE_COLLAPSE)

        def load(bv):
            n, s, st = load_rows(blk, read_rows(used[bv] - 1))
            return (n, s, st, *blk.scan())

        def burden(grp_ptr, var_idx, flip, mean, W):
            with np.errstate(invalid="ignore"):
                return blk.burden(grp_ptr, var_idx, flip, W, mean[:, None] * W)

        if kmat is None:
            skat = (lambda *a: (*blk.skat(*a), None)) if hasattr(blk, "skat") else None
        else:
            if not hasattr(blk, "skat_kmat"):
                raise NotImplementedError(NO_DOSAGE_KMAT.format("SKAT"))
            op = stack.enter_context(kmat.operator(pr.sc))
            skat = lambda *a: blk.skat_kmat(op, *a, *kmat.args)      # noqa: E731
        yield SimpleNamespace(batches=batches, load=load, burden=burden, skat=skat, collapse=getattr(blk, "collapse", None))


SkatStep = collections.namedtuple("SkatStep", "kept unit_ptr var_idx flip mean score cov n_iter")
NO_DOSAGE_SKAT = "SKAT on dosage input is not implemented."
NO_DOSAGE_COLLAPSE = "'collapse_mac' on dosage input needs a dosage block with collapse."


def skat_step(pr: _Prepared, skat, rows, bv) -> SkatStep:
    """SKAT's device step for the units whose variants are ``rows`` (per unit, rows of the per-variant arrays), all of
    them resident as ``bv``.  ``kept``: per unit the variants in the test, those that pass the scan with mac > 0;
    ``unit_ptr`` / ``var_idx``: the same as CSR over the resident rows; ``flip`` / ``mean``: the scan's own imputation
    and flip, from the double sum ``s`` -- not from the truncated sum, which is a quirk of the reference's burden code
    only; ``score`` / ``cov`` / ``n_iter``: what the backend's ``skat`` returns for them."""
    ok = (pr.valid != 0) & (pr.mac > 0)
    kept = [r[ok[r]] for r in rows]
    rows_k = np.concatenate(kept)
    unit_ptr = np.concatenate([[0], np.cumsum([k.size for k in kept])]).astype(np.int64)
    var_idx = np.searchsorted(bv, rows_k).astype(np.int32)
    flip, mean = flip_mean(pr.n[rows_k], pr.s[rows_k])
    return SkatStep(kept, unit_ptr, var_idx, flip, mean, *skat(unit_ptr, var_idx, flip, mean))


def check_collapse_mac(collapse_mac) -> float:
    """``collapse_mac`` of the SKAT drivers: NaN (off) or a number of at least 1."""
    if not _is_num(collapse_mac):
        raise TypeError("is.numeric(collapse.mac) is not TRUE")
    collapse_mac = float(collapse_mac)
    if not (math.isnan(collapse_mac) or collapse_mac >= 1):
        raise ValueError("'collapse_mac' should be NaN (no collapsing) or at least 1.")
    return collapse_mac


def collapse_step(pr: _Prepared, collapse, bt, rows, bv):
    """The ultra-rare variants of the units ``bt`` become one pseudo-variant a unit, before ``skat_step``:
    of a unit's variants in the test (valid, mac > 0) those with mac <= pr.collapse_mac are its set U; where U is not
    empty the backend's ``collapse`` makes the row of per-sample maxima of U's minor-allele dosages -- the flip is the
    scan's own, ``flip_mean`` -- and scans it.  The pseudo-variants get rows of the per-variant arrays after all others
    (pr.pseudo[u]; pr.n_collapsed[u] = |U|) and take U's place at the end of the unit -> (rows, bv) for ``skat_step``."""
    rare = (pr.valid != 0) & (pr.mac > 0) & (pr.mac <= pr.collapse_mac)
    U = [r[rare[r]] for r in rows]
    sizes = np.array([u.size for u in U])
    pr.n_collapsed[bt] = sizes
    if not sizes.any():
        return rows, bv
    ent = np.concatenate(U)
    grp_ptr = np.concatenate([[0], np.cumsum(sizes[sizes > 0])]).astype(np.int64)
    n, s, _, out, valid = collapse(grp_ptr, np.searchsorted(bv, ent).astype(np.int32), flip_mean(pr.n[ent], pr.s[ent])[0])
    new = pr.n.size + np.arange(n.size)
    maf, mac, pval = variant_stats(n.astype(np.float64), s, out, valid)
    for nm, x in (("n", n), ("s", s), ("out", out), ("valid", valid), ("maf", maf), ("mac", mac), ("pval", pval)):
        setattr(pr, nm, np.concatenate([getattr(pr, nm), x]))
    pr.pseudo[np.asarray(bt)[sizes > 0]] = new
    own = iter(new)
    return [np.append(r[~rare[r]], next(own)) if k else r for r, k in zip(rows, sizes)], np.concatenate([bv, new])


def _burden_entries(pr: _Prepared, rows, bv, n, st, kinds, burden_mac):
    """``ds_mat_burden`` (src/saige_main.cpp:526-610) up to the collapse itself, for the units whose variants are
    ``rows``: per unit a group of entries (the variants with a weight in any column) -> (grp_ptr, var_idx into the
    resident rows bv, flip, mean, W [entries, kinds x weight sets]).  Column kind "all": weights dbeta(maf); "rare",
    ACAT-V's burden of the rare variants: the same where mac < burden_mac (mac >= threshold -> single-variant test, not
    in the burden).  The weights are normalised per column (``f64_normalize``); the mean and the flip come from the
    reference's `int sum` ``st``."""
    grp_ptr, var_idx, flip, mean, ws = [0], [], [], [], []
    for r in rows:
        cols = []
        for kind in kinds:
            keep = pr.mac[r] < burden_mac if kind == "rare" else True
            cols += [np.where(keep, _dbeta(pr.maf[r], a, b), np.nan) for a, b in pr.wbeta.T]
        W = np.array(cols, dtype=np.float64).reshape(len(cols), len(r)).T.copy()
        for c in range(W.shape[1]):
            fin = np.isfinite(W[:, c])
            sm = W[fin, c].sum()
            if sm > 0:
                W[fin, c] = W[fin, c] * (1 / sm)                   # f64_normalize
        p = np.searchsorted(bv, r)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = st[p] / n[p]                                       # (double)sum / n
        fl = st[p] > n[p]
        keep = np.isfinite(W).any(axis=1)
        var_idx.append(p[keep])
        flip.append(fl[keep])
        mean.append(np.where(fl, 2 - m, m)[keep])
        ws.append(W[keep])
        grp_ptr.append(grp_ptr[-1] + int(keep.sum()))
    return (grp_ptr, np.concatenate(var_idx).astype(np.int32), np.concatenate(flip).astype(np.uint8), np.concatenate(mean),
            np.concatenate(ws).reshape(-1, len(kinds) * pr.wbeta.shape[1]))


def _run(pr: _Prepared, kinds=(), burden_mac=float("nan"), skat=False):
    """The device side of a driver call, per batch of units of the rows backend: load the batch's distinct variants,
    fill the per-variant arrays, then SKAT's step (``skat``: pr.skat gets one ``SkatStep`` per batch; with pr.collapse_mac
    after ``collapse_step``, which appends the pseudo-variants to the per-variant arrays) and one burden call
    with every column of the driver (``kinds``: pr.burden[kind] = (rows [n_units, n_weights, 8], valid))."""
    nu, nw, nv = len(pr.index), pr.wbeta.shape[1], np.unique(np.concatenate(pr.index)).size
    pr.n, pr.s, pr.out, pr.valid = np.zeros(nv), np.zeros(nv), np.full((nv, 8), np.nan), np.zeros(nv, dtype=np.uint8)
    pr.maf, pr.mac, pr.pval = np.full(nv, np.nan), np.full(nv, np.nan), np.full(nv, np.nan)
    rows_out, rows_valid = np.full((nu, len(kinds) * nw, 8), np.nan), np.zeros((nu, len(kinds) * nw), dtype=np.uint8)
    pr.skat = [] if skat else None
    collapsing = skat and not math.isnan(pr.collapse_mac)
    if collapsing:
        pr.n_collapsed, pr.pseudo = np.zeros(nu, dtype=np.int64), np.full(nu, -1, dtype=np.int64)
    with pr.backend as be:
        if skat and be.skat is None:
            raise NotImplementedError(NO_DOSAGE_SKAT)
        if collapsing and be.collapse is None:
            raise NotImplementedError("'collapse_mac' needs a scanner with collapse_2bit.")
        for bt in be.batches:
            rows = [pr.index[u] for u in bt]
            bv = np.unique(np.concatenate(rows))                    # rows of the per-variant arrays
            n, s, st, out, valid = be.load(bv)
            n = n.astype(np.float64)
            pr.n[bv], pr.s[bv], pr.out[bv], pr.valid[bv] = n, s, out, valid
            pr.maf[bv], pr.mac[bv], pr.pval[bv] = variant_stats(n, s, out, valid)
            if skat:
                pr.skat.append(skat_step(pr, be.skat, *(collapse_step(pr, be.collapse, bt, rows, bv) if collapsing else (rows, bv))))
            if kinds:
                ob, vb = be.burden(*_burden_entries(pr, rows, bv, n, st, kinds, burden_mac))
                rows_out[bt], rows_valid[bt] = ob.reshape(len(bt), -1, 8), vb.reshape(len(bt), -1)
    pr.burden = {kind: (rows_out[:, k * nw:(k + 1) * nw], rows_valid[:, k * nw:(k + 1) * nw]) for k, kind in enumerate(kinds)}


def _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, what, scanner_factory=None, dsnode="",
             ds_budget=None, kmat=None, collapse_mac=float("nan")) -> _Prepared:
    """Common head of the set-test drivers (R/assoc_aggregate.r:55-150): checks, sample matching, the model, the scanner
    and the rows backend of the input (and what the reference prints about the units).  Nothing has gone to the device
    yet: ``_run`` does that.  ``collapse_mac`` (SKAT and SKAT-O; what ``check_collapse_mac`` returned)
    other than NaN on dosage input needs a scanner whose dosage blocks collapse: the factory (``Scanner`` when None) must
    be a class that says so (``ds_collapse = True``); anything else is refused here, before the scanner is made."""
    if verbose:
        print(what)
    pr = _Prepared(_Units(units), _check_beta(wbeta), collapse_mac=collapse_mac)
    for nm, v in (("spa.pval", spa_pval), ("var.ratio", var_ratio)):
        if not _is_num(v):
            raise TypeError(f"is.numeric({nm}) is not TRUE")
    mod: NullModel = load_modobj(modobj, verbose)
    no_loco(mod, what.rstrip(":"))
    pr.inp = inp = reduce_hard_calls(open_scan_input(gdsfile, mod, dsnode, verbose))
    if inp.kind != "packed" and not math.isnan(pr.collapse_mac):
        fac = Scanner if scanner_factory is None else scanner_factory
        if not (isinstance(fac, type) and getattr(fac, "ds_collapse", False)):
            raise NotImplementedError("'collapse_mac' on dosage input is not implemented.")
    used = np.unique(np.concatenate(pr.units.index))
    if used.size == 0 or used.min() < 1 or used.max() > inp.n_var:
        raise ValueError("No variant in the genotypic data set!")
    pr.index = [np.searchsorted(used, ix) for ix in pr.units.index]
    if not math.isfinite(var_ratio):
        var_ratio = float(np.nanmean(mod.var_ratio))
    sizes = np.array([len(ix) for ix in pr.units.index])
    if verbose:
        print(f"    # of samples: {pr.inp.n_samp:,}")
        print(f"    # of variants in total: {used.size:,}")
        print(f"    # of units: {len(pr.units.index):,}")
        print(f"    avg. # of variants per unit: {sizes.mean()}")
        print(f"    min # of variants in a unit: {sizes.min()}")
        print(f"    max # of variants in a unit: {sizes.max()}")
        print(f"    p-value threshold for SPA adjustment: {spa_pval}")
        print(f"    variance ratio for approximation: {var_ratio}")
        print("    variant weights: " + ", ".join(f"beta({a:g},{b:g})" for a, b in pr.wbeta.T))
    # .init_nullmod(modobj, ii, 0, 0, 1, spa.pval, var.ratio, ...): maf 0, mac 0, missing 1
    pr.sm = init_nullmod(mod, pr.inp.ii, 0.0, 0.0, 1.0, spa_pval, var_ratio)
    pr.binary = mod.trait_type == "binary"
    pr.wb_colnm = [f"b{a:g}_{b:g}" for a, b in pr.wbeta.T]
    pr.sc = Scanner(pr.sm) if scanner_factory is None else scanner_factory(pr.sm)   # tests inject the CPU oracle
    if verbose:
        print("Calculating p-values:")
    if inp.kind == "packed":
        pr.backend = _packed_rows(pr, used, kmat)
    else:
        pr.backend = _dosage_rows(pr, used, inp.stored_ok(scanner_factory), DS_BUDGET if ds_budget is None else ds_budget,
                                  kmat)
    return pr


def _summary_cols(pr: _Prepared) -> Dict[str, Any]:
    ans: Dict[str, Any] = dict(pr.units.desp)
    ans["numvar"] = np.array([len(r) for r in pr.index])
    st = np.array([[*_mean_sd(pr.maf[r]), *_minmax(pr.maf[r]), *_mean_sd(pr.mac[r]), *_minmax(pr.mac[r])] for r in pr.index])
    for k, nm in enumerate(("maf.avg", "maf.sd", "maf.min", "maf.max", "mac.avg", "mac.sd", "mac.min", "mac.max")):
        ans[nm] = st[:, k]
    return ans


def _collapse_cols(pr: _Prepared, ans: Dict[str, Any]):
    """The two columns of a call with ``collapse_mac``: ``n.collapsed``, the variants a unit's pseudo-variant replaces,
    and ``mac.collapsed``, the pseudo-variant's minor allele count (NaN: the unit has none)."""
    if pr.n_collapsed is not None:
        ans["n.collapsed"] = pr.n_collapsed
        ans["mac.collapsed"] = np.where(pr.pseudo >= 0, pr.mac[pr.pseudo], np.nan)


def _row_result(o, ok, n_snp, summac_thr):
    """[summac, beta, SE, pval, p.norm, cvg] of one burden row: saige_burden_test_bin, :640-665."""
    summac = (2 * o[2] * o[0]) * n_snp if np.isfinite(o[0]) else 0.0   # f64_sum(G) * n_snp
    if not ok or not (summac >= summac_thr and summac > 0):
        return summac, float("nan"), float("nan"), float("nan"), float("nan"), 0.0
    return summac, o[3], o[4], o[5], o[6], o[7]


def seqAssocGLMM_spaBurden(gdsfile, modobj, units, wbeta=AggrParamBeta, summac: float = 3, dsnode: str = "",
                           spa_pval: float = 0.05, var_ratio: float = float("nan"), res_savefn: str = "",
                           res_compress: str = "LZMA", parallel=False, verbose: bool = True,
                           verbose_maf: bool = True, scanner_factory=None,
                           ds_budget: Optional[int] = None) -> Dict[str, Any]:
    """Burden tests per unit and weight set (R/assoc_aggregate.r:51-302)."""
    if not (_is_num(summac) and math.isfinite(summac)):
        raise TypeError("is.finite(summac) is not TRUE")
    pr = _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, "SAIGE burden analysis:", scanner_factory,
                  dsnode, ds_budget)
    try:
        _run(pr, ("all",))
    finally:
        pr.sc.close()
    ans = _summary_cols(pr)
    out, valid = pr.burden["all"]
    for i, nm in enumerate(pr.wb_colnm):
        sfx = f".{nm}" if len(pr.wb_colnm) > 1 else ""
        res = np.array([_row_result(out[u, i], valid[u, i], len(r), summac) for u, r in enumerate(pr.index)])
        ans["summac" + sfx], ans["beta" + sfx], ans["SE" + sfx], ans["pval" + sfx] = res[:, 0], res[:, 1], res[:, 2], res[:, 3]
        if pr.binary:
            ans["p.norm" + sfx] = res[:, 4]
            ans["cvg" + sfx] = res[:, 5] != 0
    _save(ans, res_savefn, res_compress, verbose)
    return ans


def _acatv(pr: _Prepared, burden_mac: float, burden_summac: float):
    """ACAT-V per unit and weight set (saige_acatv_test_bin, src/saige_main.cpp:720-830):
    returns p [n_units, n_w], and (n.single, n.burden, median/min/max of the combined p-values)."""
    nu, nw = len(pr.index), pr.wbeta.shape[1]
    out, valid = pr.burden["rare"]
    p = np.full((nu, nw), np.nan)
    extra = np.full((nu, 2 + 3 * nw), np.nan)
    for u, r in enumerate(pr.index):
        single = pr.mac[r] >= burden_mac
        n_burden = int((~single).sum())
        has_b = np.isfinite(_dbeta(pr.maf[r][~single], *pr.wbeta[:, 0])).any()      # a rare variant with a weight
        for i, (a, b) in enumerate(pr.wbeta.T):
            mf = pr.maf[r][single]
            pv = list(pr.pval[r][single])
            wp = list(_dbeta(mf, a, b) ** 2 * mf * (1 - mf))
            if has_b:
                sm, _, _, pb, _, _ = _row_result(out[u, i], valid[u, i], len(r), burden_summac)
                if np.isfinite(pb):
                    pm = pr.maf[r][~single].sum() / n_burden
                    wp.append(float(_dbeta(pm, a, b)) ** 2 * pm * (1 - pm))
                    pv.append(pb)
            if i == 0:
                extra[u, 0] = len(pv) - n_burden
                extra[u, 1] = n_burden
            p[u, i] = acat_pval(pv, wp) if pv else float("nan")
            fin = np.asarray(pv, dtype=np.float64)
            fin = fin[np.isfinite(fin)]
            if fin.size:
                extra[u, 2 + 3 * i: 5 + 3 * i] = [np.median(fin), fin.min(), fin.max()]
    return p, extra


def seqAssocGLMM_spaACAT_V(gdsfile, modobj, units, wbeta=AggrParamBeta, burden_mac: float = 10,
                           burden_summac: float = 3, dsnode: str = "", spa_pval: float = 0.05,
                           var_ratio: float = float("nan"), res_savefn: str = "", res_compress: str = "LZMA",
                           parallel=False, verbose: bool = True, verbose_maf: bool = True, scanner_factory=None,
                           ds_budget: Optional[int] = None) -> Dict[str, Any]:
    """ACAT-V tests (R/assoc_aggregate.r:309-557); binary outcomes only, as in the reference."""
    pr = _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, "SAIGE ACAT-V analysis:", scanner_factory,
                  dsnode, ds_budget)
    try:
        if not pr.binary:
            raise NotImplementedError("'saige_acatv_test_quant' not implemented.")
        _run(pr, ("rare",), burden_mac)
    finally:
        pr.sc.close()
    ans = _summary_cols(pr)
    p, extra = _acatv(pr, burden_mac, burden_summac)
    ans["n.single"], ans["n.burden"] = extra[:, 0].astype(np.int64), extra[:, 1].astype(np.int64)
    for i, nm in enumerate(pr.wb_colnm):
        sfx = f".v{nm[1:]}" if len(pr.wb_colnm) > 1 else ""      # wb_colnm = "v%g_%g", R/assoc_aggregate.r:389
        ans["pval" + sfx] = p[:, i]
        ans["p.med" + sfx], ans["p.min" + sfx], ans["p.max" + sfx] = extra[:, 2 + 3 * i], extra[:, 3 + 3 * i], extra[:, 4 + 3 * i]
    _save(ans, res_savefn, res_compress, verbose)
    return ans


def seqAssocGLMM_spaACAT_O(gdsfile, modobj, units, wbeta=AggrParamBeta, burden_mac: float = 10,
                           burden_summac: float = 3, dsnode: str = "", spa_pval: float = 0.05,
                           var_ratio: float = float("nan"), res_savefn: str = "", res_compress: str = "LZMA",
                           parallel=False, verbose: bool = True, verbose_maf: bool = True, scanner_factory=None,
                           ds_budget: Optional[int] = None) -> Dict[str, Any]:
    """ACAT-O: burden and ACAT-V p-values of every weight set combined by ACAT
    (R/assoc_aggregate.r:564-797, saige_acato_test_bin src/saige_main.cpp:845-976)."""
    pr = _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, "SAIGE ACAT-O analysis:", scanner_factory,
                  dsnode, ds_budget)
    try:
        if not pr.binary:
            raise NotImplementedError("'saige_acato_test_quant' not implemented.")
        _run(pr, ("all", "rare"), burden_mac)
    finally:
        pr.sc.close()
    ans = _summary_cols(pr)
    out, valid = pr.burden["all"]
    pb = np.array([[_row_result(out[u, i], valid[u, i], len(r), burden_summac)[3] for i in range(pr.wbeta.shape[1])]
                   for u, r in enumerate(pr.index)])
    pv, _ = _acatv(pr, burden_mac, burden_summac)
    both = np.empty((pb.shape[0], 2 * pb.shape[1]))
    both[:, 0::2], both[:, 1::2] = pb, pv
    ans["pval"] = np.array([acat_pval(row) for row in both])
    for i, nm in enumerate(pr.wb_colnm):
        ans["pval.b" + nm[1:]] = pb[:, i]
        ans["pval.v" + nm[1:]] = pv[:, i]
    _save(ans, res_savefn, res_compress, verbose)
    return ans


def _save(ans, res_savefn, res_compress, verbose):
    if not res_savefn:
        if verbose:
            print("Done.")
        return
    import re
    from .results import save_result
    if re.search(r"\.(rda|RData)$", res_savefn, re.I):
        if verbose:
            print(f"Save to '{res_savefn}' ...")
        save_result({k: v for k, v in ans.items()}, res_savefn, "ZIP" if res_compress == "none" else res_compress)
    else:
        raise ValueError("Unknown format of the output file, and it should be RData or gds.")
