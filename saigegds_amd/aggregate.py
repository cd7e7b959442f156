"""Aggregate tests on MI355X: burden, ACAT-V and ACAT-O.

Python mirror of ``seqAssocGLMM_spaBurden()``, ``seqAssocGLMM_spaACAT_V()``,
``seqAssocGLMM_spaACAT_O()`` and ``pACAT()`` (reference R/assoc_aggregate.r:51-797,
native side src/saige_main.cpp:466-1052).  The reference calls one native routine per
unit; here the work of ALL units goes through the scan library in three batches:

1. one ``sgx_scan_2bit`` over every variant that occurs in a unit (thresholds 0 / 0 / 1 as
   ``.init_nullmod(modobj, ii, 0, 0, 1, ...)`` sets them): its AF / num columns give the
   per-variant maf and mac of ``ds_mat_mafmac`` and its p-values are the single-variant
   tests of ACAT-V;
2. one ``sgx_burden_2bit`` over all (unit, weight) burden rows: the weighted, mean-imputed,
   minor-allele-oriented collapse of ``ds_mat_burden`` is a device kernel, followed on the
   device by the same single-variant test;
3. the Cauchy combination (``acat_pval``) on the host.

That is the flow of 2-bit genotypes (``$dosage_alt``, the RAW branch of the reference routines).  Dosage
input -- a format node such as ``annotation/format/DS``, or a ``GenotypeSource(dosage=...)`` of uint8, int32 or
float64 (the INTSXP / REALSXP branches) -- goes through ``DosageBlock`` in batches of consecutive units whose
distinct variants fit a byte budget on the device: the rows of a batch are uploaded once, and counts, single-variant
tests and the burden rows of every column of the driver are made from the resident rows (``_run_dosage``); the SKAT
driver (``skat.py``) takes its score statistics and covariance matrices from the same resident rows.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ._lib import Scanner
from .assoc import PackedRows, ScanInput, _is_num, open_scan_input
from .gds import pack_dosage_2bit, unpack_dosage_2bit
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
    """What ``_prepare`` hands a set-test driver.  The per-variant arrays are indexed by ``local``."""
    units: _Units
    wbeta: np.ndarray                       # [2, n_weights]
    inp: ScanInput = None                   # the opened input
    local: Dict[int, int] = None            # 1-based variant index -> row of the per-variant arrays
    sm: ScanModel = None                    # the model at thresholds 0 / 0 / 1
    binary: bool = False
    wb_colnm: List[str] = None              # "b<a>_<b>" per weight set
    sc: Any = None                          # the scanner; the driver closes it
    n: np.ndarray = None                    # per variant: non-missing samples,
    s: np.ndarray = None                    # their sum (a double sum for real dosages),
    maf: np.ndarray = None
    mac: np.ndarray = None
    pval: np.ndarray = None                 # the single-variant p-value (NaN: rejected by the scan's filter)
    out: np.ndarray = None                  # the scan table [n, 8] and
    valid: np.ndarray = None                # its valid flags (dosage route: the SKAT driver only)
    rows: List[List[int]] = None            # per unit: rows of the per-variant arrays (_summary_cols)
    packed: np.ndarray = None               # 2-bit route: the variants' rows for the model's samples
    st: np.ndarray = None                   # dosage route: the truncated `int sum` of ds_mat_burden
    ds_out: Optional[Dict[str, Any]] = None  # dosage route: column kind -> (burden rows [n_units, n_weights, 8], valid)
    skat_rows: List[np.ndarray] = None      # dosage route, SKAT: per unit the variants in the test,
    skat_S: List[np.ndarray] = None         # their score statistics
    skat_Phi: List[np.ndarray] = None       # and covariance


def _prepare_model(pr, mod, used, spa_pval, var_ratio, verbose, scanner_factory):
    """The model and the scanner of a driver call (and what the reference prints about the units)."""
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


DS_BUDGET = 1 << 30      # bytes of dosage rows resident on the device per batch of units


def flip_mean(n, s):
    """The scan's own imputation and flip of rows from their counts (n non-missing, s their double sum) ->
    (flip = s > n as uint8, mean = s / n, or 2 - s / n where flipped)."""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s / n
    fl = s > n
    return fl.astype(np.uint8), np.where(fl, 2 - m, m)


def _sets_all(pr, r):
    """Weights of a unit's burden row per weight set: dbeta(maf)."""
    return [_dbeta(pr.maf[r], a, b) for a, b in pr.wbeta.T]


def _sets_rare(pr, r, burden_mac):
    """... of ACAT-V's burden of the rare variants: mac >= threshold -> single-variant test, not in the burden."""
    rare = pr.mac[r] < burden_mac
    return [np.where(rare, _dbeta(pr.maf[r], a, b), np.nan) for a, b in pr.wbeta.T]


def _hard_calls(ds: np.ndarray) -> bool:
    """An integer matrix that holds 0, 1, 2 and the missing code only: the RAW branch's meaning."""
    miss = 0xFF if ds.dtype == np.uint8 else np.iinfo(np.int32).min
    return bool(np.all((ds == miss) | ((ds >= 0) & (ds <= 2))))


def _run_dosage(pr, stored, used, kinds, burden_mac, budget):
    """Dosage flow: the units in batches of consecutive units whose distinct variants fit ``budget`` bytes of
    resident rows (a unit larger than that is a batch of its own).  Per batch: rows -> block (one upload), counts and
    single-variant tests into the per-variant arrays, weights, one burden call with every column of the driver.
    A variant that two batches share (sliding windows) is loaded in both.  Fills pr.n / s / maf / mac / pval and
    pr.ds_out[kind] = (rows [n_units, n_weights, 8], valid).

    Column kind ``"skat"`` (the SKAT driver's only kind) makes no burden rows: the batch's scan table is kept per
    variant (pr.out [n, 8], pr.valid), and one ``blk.skat`` call per batch gives every unit its variants with
    valid != 0 and mac > 0 (pr.skat_rows[u]), their score statistics and covariance (pr.skat_S[u], pr.skat_Phi[u]).
    Its flip and mean come from the double sum ``s`` -- what the scan's own imputation 2 AF and its flip use -- not
    from the truncated ``st``, which is a quirk of the reference's burden code only."""
    if "rare" in kinds and not pr.binary:
        return                                    # ACAT-V / ACAT-O of a quantitative trait: the driver raises, as the reference does
    read_rows, dtype = pr.inp.dosage_reader(stored), pr.inp.ds_dtype
    n_samp = pr.sm.n
    row_bytes = n_samp * (1 if np.dtype(dtype) == np.uint8 else 8)
    index = [np.array([pr.local[int(v)] for v in ix], dtype=np.int64) for ix in pr.units.index]
    batches, cur, seen = [], [], set()
    for u, r in enumerate(index):
        new = set(r.tolist()) - seen
        if cur and (len(seen) + len(new)) * row_bytes > budget:
            batches.append(cur)
            cur, seen, new = [], set(), set(r.tolist())
        cur.append(u)
        seen |= new
    batches.append(cur)
    skat = "skat" in kinds
    kinds = tuple(k for k in kinds if k != "skat")
    nv_used, nu, nw, nk = used.size, len(index), pr.wbeta.shape[1], len(kinds)
    pr.n, pr.s, pr.st = np.zeros(nv_used), np.zeros(nv_used), np.zeros(nv_used, dtype=np.int64)
    pr.maf, pr.mac, pr.pval = np.full(nv_used, np.nan), np.full(nv_used, np.nan), np.full(nv_used, np.nan)
    out_all, valid_all = np.full((nu, nk * nw, 8), np.nan), np.zeros((nu, nk * nw), dtype=np.uint8)
    cap = max(np.unique(np.concatenate([index[u] for u in bt])).size for bt in batches)
    if skat:
        pr.out, pr.valid = np.full((nv_used, 8), np.nan), np.zeros(nv_used, dtype=np.uint8)
        pr.skat_rows, pr.skat_S, pr.skat_Phi = [None] * nu, [None] * nu, [None] * nu
    with pr.sc.dosage_block(dtype, cap) as blk:
        if skat and not hasattr(blk, "skat"):
            raise NotImplementedError("SKAT on dosage input is not implemented.")
        for bt in batches:
            bv = np.unique(np.concatenate([index[u] for u in bt]))          # rows of the per-variant arrays
            rows = read_rows(used[bv] - 1)
            n, s, st = blk.load_packed(*rows.args()) if isinstance(rows, PackedRows) else blk.load(rows)
            out, valid = blk.scan()
            n = n.astype(np.float64)
            # ds_mat_mafmac (src/saige_main.cpp:485-524): n non-missing, s their sum (a double sum for REAL dosages)
            with np.errstate(invalid="ignore", divide="ignore"):
                af = s / (2 * n)
            pr.n[bv], pr.s[bv], pr.st[bv] = n, s, st
            pr.maf[bv] = np.where(n > 0, np.minimum(af, 1 - af), np.nan)
            pr.mac[bv] = np.minimum(s, 2 * n - s)
            pr.pval[bv] = np.where(valid != 0, out[:, 5], np.nan)          # single_test_*: NaN when the filter rejects
            # ds_mat_burden (:526-610): the mean and the flip from its `int sum` (st), weights normalised per column
            loc = {int(v): k for k, v in enumerate(bv)}
            if skat:
                pr.out[bv], pr.valid[bv] = out, valid
                ok = (pr.valid != 0) & (pr.mac > 0)
                kept = [index[u][ok[index[u]]] for u in bt]
                rows_k = np.concatenate(kept)
                unit_ptr = np.concatenate([[0], np.cumsum([k.size for k in kept])])
                score, cov = blk.skat(unit_ptr, np.array([loc[int(v)] for v in rows_k], dtype=np.int32),
                                      *flip_mean(pr.n[rows_k], pr.s[rows_k]))
                for k, u in enumerate(bt):
                    pr.skat_rows[u], pr.skat_Phi[u] = kept[k], np.array(cov[k], dtype=np.float64)
                    pr.skat_S[u] = np.array(score[unit_ptr[k]:unit_ptr[k + 1]], dtype=np.float64)
            if not kinds:
                continue
            grp_ptr, var_idx, flip, ws, mws = [0], [], [], [], []
            for u in bt:
                r = index[u]
                cols = []
                for kind in kinds:
                    cols += _sets_all(pr, r) if kind == "all" else _sets_rare(pr, r, burden_mac)
                W = np.array(cols, dtype=np.float64).reshape(nk * nw, len(r)).T.copy()
                for c in range(W.shape[1]):
                    fin = np.isfinite(W[:, c])
                    sm = W[fin, c].sum()
                    if sm > 0:
                        W[fin, c] = W[fin, c] * (1 / sm)                   # f64_normalize
                with np.errstate(invalid="ignore", divide="ignore"):
                    m = pr.st[r] / pr.n[r]                                 # (double)sum / n
                fl = pr.st[r] > pr.n[r]
                m = np.where(fl, 2 - m, m)
                keep = np.isfinite(W).any(axis=1)
                var_idx += [loc[int(v)] for v in r[keep]]
                flip += list(fl[keep])
                ws.append(W[keep])
                with np.errstate(invalid="ignore"):
                    mws.append(m[keep, None] * W[keep])
                grp_ptr.append(len(var_idx))
            ob, vb = blk.burden(grp_ptr, np.asarray(var_idx, dtype=np.int32), np.asarray(flip, dtype=np.uint8),
                                np.concatenate(ws).reshape(-1, nk * nw), np.concatenate(mws).reshape(-1, nk * nw))
            out_all[bt] = ob.reshape(len(bt), nk * nw, 8)
            valid_all[bt] = vb.reshape(len(bt), nk * nw)
    pr.ds_out = {kind: (out_all[:, k * nw:(k + 1) * nw], valid_all[:, k * nw:(k + 1) * nw]) for k, kind in enumerate(kinds)}


def _prepare(gdsfile, modobj, units, wbeta, spa_pval, var_ratio, verbose, what, scanner_factory=None, dsnode="",
             kinds=("all",), burden_mac=float("nan"), ds_budget=None) -> _Prepared:
    """Common head of the three drivers (R/assoc_aggregate.r:55-150): checks, sample matching,
    model, and the per-variant scan of every variant that occurs in a unit.  Dosage input: the whole
    device side, the burden rows of the driver's column ``kinds`` included (``_run_dosage``)."""
    if verbose:
        print(what)
    pr = _Prepared(_Units(units), _check_beta(wbeta))
    for nm, v in (("spa.pval", spa_pval), ("var.ratio", var_ratio)):
        if not _is_num(v):
            raise TypeError(f"is.numeric({nm}) is not TRUE")
    mod: NullModel = load_modobj(modobj, verbose)
    no_loco(mod, what.rstrip(":"))
    inp = open_scan_input(gdsfile, mod, dsnode, verbose)
    if inp.kind == "dosage" and inp.in_mem and inp.ds_dtype != np.float64 and _hard_calls(inp.ds_all):
        # hard calls: the reference's RAW branch has the same meaning -> the 2-bit path
        codes = np.where((inp.ds_all < 0) | (inp.ds_all > 2), 3, inp.ds_all).astype(np.uint8)
        inp = dataclasses.replace(inp, kind="packed", packed=pack_dosage_2bit(codes), ds_all=None, ds_dtype=None)
    pr.inp = inp
    used = np.unique(np.concatenate(pr.units.index))
    if used.size == 0 or used.min() < 1 or used.max() > inp.n_var:
        raise ValueError("No variant in the genotypic data set!")
    pr.local = {int(v): k for k, v in enumerate(used)}
    if inp.kind != "packed":
        _prepare_model(pr, mod, used, spa_pval, var_ratio, verbose, scanner_factory)
        try:
            _run_dosage(pr, inp.stored_ok(scanner_factory), used, kinds, burden_mac, DS_BUDGET if ds_budget is None else ds_budget)
        except BaseException:
            pr.sc.close()
            raise
        return pr
    pr.packed = packed = inp.packed_rows_at(used - 1)
    _prepare_model(pr, mod, used, spa_pval, var_ratio, verbose, scanner_factory)
    out, valid = pr.sc.scan_2bit(packed)
    # ds_mat_mafmac (src/saige_main.cpp:466-524), RAW branch: n non-missing, s = sum of codes
    num = out[:, 2]
    # a variant rejected by the scan's filter (monomorphic: maf = 0) still has counts: redo them on the host
    codes = None
    if (valid == 0).any():
        codes = unpack_dosage_2bit(packed[valid == 0], inp.n_samp).astype(np.int64)
    n = np.where(valid != 0, num, 0).astype(np.float64)
    s = np.where(valid != 0, np.rint(out[:, 0] * 2 * np.where(valid != 0, num, 0)), 0.0)
    if codes is not None:
        nm = (codes != 3).sum(axis=1)
        sm_ = np.where(codes != 3, codes, 0).sum(axis=1)
        n[valid == 0] = nm
        s[valid == 0] = sm_
    with np.errstate(invalid="ignore", divide="ignore"):
        af = s / (2 * n)
    pr.n, pr.s = n, s
    pr.maf = np.where(n > 0, np.minimum(af, 1 - af), np.nan)
    pr.mac = np.minimum(s, 2 * n - s)
    pr.pval = np.where(valid != 0, out[:, 5], np.nan)          # single_test_*: NaN when the filter rejects
    pr.out, pr.valid = out, valid                               # the whole table: the SKAT driver's SPA adjustment
    return pr


def _summary_cols(pr: _Prepared) -> Dict[str, Any]:
    ans: Dict[str, Any] = dict(pr.units.desp)
    rows = [[pr.local[int(v)] for v in ix] for ix in pr.units.index]
    pr.rows = rows
    ans["numvar"] = np.array([len(r) for r in rows])
    st = np.array([[*_mean_sd(pr.maf[r]), *_minmax(pr.maf[r]), *_mean_sd(pr.mac[r]), *_minmax(pr.mac[r])] for r in rows])
    for k, nm in enumerate(("maf.avg", "maf.sd", "maf.min", "maf.max", "mac.avg", "mac.sd", "mac.min", "mac.max")):
        ans[nm] = st[:, k]
    return ans


def _burden_rows(pr: _Prepared, weight_sets: List[List[np.ndarray]], kind: str = "all"):
    """weight_sets[u][k] = per-variant weights (NaN = not in the burden) of unit u, row kind k.
    Returns the scan rows [n_units, n_kinds, 8] and validity; ``f64_normalize`` and the tables of
    ``ds_mat_burden`` (RAW branch) are formed here.  Dosage input: the rows of column kind ``kind`` were
    made while their batch was resident (``_run_dosage``, from the same weights)."""
    if pr.ds_out is not None:
        return pr.ds_out[kind]
    row_ptr, var_idx, lut = [0], [], []
    for u, sets in enumerate(weight_sets):
        r = np.asarray(pr.rows[u])
        for w in sets:
            w = np.asarray(w, dtype=np.float64).copy()
            fin = np.isfinite(w)
            sm = w[fin].sum()
            if sm > 0:
                w[fin] = w[fin] * (1 / sm)                         # f64_normalize
            for j in np.flatnonzero(fin):
                v = r[j]
                n, s = pr.n[v], pr.s[v]
                m = s / n if n > 0 else float("nan")             # (double)sum / n
                if s <= n:
                    t = [0 * w[j], 1 * w[j], 2 * w[j], m * w[j]]
                else:
                    t = [2 * w[j], 1 * w[j], 0 * w[j], (2 - m) * w[j]]
                var_idx.append(v)
                lut.append(t)
            row_ptr.append(len(var_idx))
    lut_a = np.asarray(lut, dtype=np.float64).reshape(-1, 4)
    out, valid = pr.sc.burden_2bit(pr.packed, np.asarray(row_ptr), np.asarray(var_idx, dtype=np.int32), lut_a)
    nk = len(weight_sets[0]) if weight_sets else 0
    return out.reshape(len(weight_sets), nk, 8), valid.reshape(len(weight_sets), nk)


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
                  dsnode, ("all",), ds_budget=ds_budget)
    try:
        ans = _summary_cols(pr)
        sets = [_sets_all(pr, r) for r in pr.rows]
        out, valid = _burden_rows(pr, sets)
    finally:
        pr.sc.close()
    for i, nm in enumerate(pr.wb_colnm):
        sfx = f".{nm}" if len(pr.wb_colnm) > 1 else ""
        res = np.array([_row_result(out[u, i], valid[u, i], len(pr.rows[u]), summac) for u in range(len(pr.rows))])
        ans["summac" + sfx], ans["beta" + sfx], ans["SE" + sfx], ans["pval" + sfx] = res[:, 0], res[:, 1], res[:, 2], res[:, 3]
        if pr.binary:
            ans["p.norm" + sfx] = res[:, 4]
            ans["cvg" + sfx] = res[:, 5] != 0
    _save(ans, res_savefn, res_compress, verbose)
    return ans


def _acatv(pr: _Prepared, burden_mac: float, burden_summac: float):
    """ACAT-V per unit and weight set (saige_acatv_test_bin, src/saige_main.cpp:720-830):
    returns p [n_units, n_w], and (n.single, n.burden, median/min/max of the combined p-values)."""
    nu, nw = len(pr.rows), pr.wbeta.shape[1]
    sets = [_sets_rare(pr, r, burden_mac) for r in pr.rows]
    has_b = [bool(np.isfinite(s[0]).any()) for s in sets]
    out, valid = _burden_rows(pr, sets, "rare")
    p = np.full((nu, nw), np.nan)
    extra = np.full((nu, 2 + 3 * nw), np.nan)
    for u, r in enumerate(pr.rows):
        r = np.asarray(r)
        single = pr.mac[r] >= burden_mac
        n_burden = int((~single).sum())
        for i, (a, b) in enumerate(pr.wbeta.T):
            mf = pr.maf[r][single]
            pv = list(pr.pval[r][single])
            wp = list(_dbeta(mf, a, b) ** 2 * mf * (1 - mf))
            if has_b[u]:
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
                  dsnode, ("rare",), burden_mac, ds_budget)
    try:
        if not pr.binary:
            raise NotImplementedError("'saige_acatv_test_quant' not implemented.")
        ans = _summary_cols(pr)
        p, extra = _acatv(pr, burden_mac, burden_summac)
    finally:
        pr.sc.close()
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
                  dsnode, ("all", "rare"), burden_mac, ds_budget)
    try:
        if not pr.binary:
            raise NotImplementedError("'saige_acato_test_quant' not implemented.")
        ans = _summary_cols(pr)
        sets = [_sets_all(pr, r) for r in pr.rows]
        out, valid = _burden_rows(pr, sets)
        pb = np.array([[_row_result(out[u, i], valid[u, i], len(pr.rows[u]), burden_summac)[3]
                        for i in range(pr.wbeta.shape[1])] for u in range(len(pr.rows))])
        pv, _ = _acatv(pr, burden_mac, burden_summac)
    finally:
        pr.sc.close()
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
