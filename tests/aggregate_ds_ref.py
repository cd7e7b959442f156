"""CPU restatement of the reference's aggregate tests on dosage matrices -- TEST INFRASTRUCTURE ONLY.

The INTSXP and REALSXP branches of ``ds_mat_mafmac`` / ``ds_mat_burden`` (src/saige_main.cpp:485-610), unit by
unit, on top of ``oracle.Oracle.scan_f64`` for the single-variant test -- the dosage twin of
oracle/aggregate_oracle.py (RAW branch), whose weight, ACAT and single-test helpers are reused.  The REALSXP branch
of ``ds_mat_burden`` keeps its sum in an ``int`` (:589-591): ``trunc_sum`` restates that statement by statement.

``NumpyDsScanner`` gives the aggregate driver the three operations of ``saigegds_amd._lib.DosageBlock`` in numpy, so
that its host logic (batching, weights, tables, combination) runs without a GPU.
"""
import itertools
import math

import numpy as np

from oracle.aggregate_oracle import acat_pval, dbeta, normalize, single
from oracle.oracle import OracleScanner

NA_INT = np.iinfo(np.int32).min


def ok_mask(row):
    if row.dtype == np.uint8:
        return row != 0xFF
    if row.dtype == np.int32:
        return row != NA_INT
    return np.isfinite(row)


def trunc_sum(row):
    """``int sum = 0; for (j) if (ok) sum += s[j];`` -- for doubles the compound assignment converts the double
    result back to int after every addition."""
    vals = row[ok_mask(row)]
    if row.dtype != np.float64:
        return int(vals.astype(np.int64).sum())
    acc = 0
    for acc in itertools.accumulate(vals.tolist(), lambda a, x: int(a + x), initial=0):
        pass
    return acc


def ds_mat_mafmac(ds):
    maf, mac = [], []
    for row in ds:
        ok = ok_mask(row)
        n = int(ok.sum())
        if row.dtype == np.float64:
            s = float(np.cumsum(row[ok])[-1]) if n else 0.0          # double s, added sample by sample
        else:
            s = int(row[ok].astype(np.int64).sum())
        af = s / (2 * n) if n > 0 else float("nan")
        maf.append(min(af, 1 - af) if n > 0 else float("nan"))
        mac.append(float(min(s, 2 * n - s)))
    return np.array(maf), np.array(mac)


def ds_mat_burden(ds, weight, tsum=None):
    out = np.zeros(ds.shape[1])
    for j, (row, w) in enumerate(zip(ds, weight)):
        if not math.isfinite(w):
            continue
        ok = ok_mask(row)
        n = int(ok.sum())
        s = trunc_sum(row) if tsum is None else tsum[j]
        with np.errstate(invalid="ignore", divide="ignore"):
            m = float(np.float64(s) / np.float64(n))
        if row.dtype == np.float64:
            r, r2 = np.where(ok, row, 0.0), np.where(ok, 2 - np.where(ok, row, 0.0), 0.0)
        else:
            ri = np.where(ok, row, 0).astype(np.int64)
            r, r2 = ri.astype(np.float64), (2 - ri).astype(np.float64)       # 2 - s[j] in integers
        with np.errstate(invalid="ignore"):
            if s <= n:
                out += np.where(ok, r * w, m * w)
            else:
                m = 2 - m
                out += np.where(ok, r2 * w, m * w)
    return out


def as_f64(row):
    g = row.astype(np.float64)
    g[~ok_mask(row)] = np.nan
    return g


def burden_unit(oracle, ds, wbeta, summac_thr):
    """-> per weight set (summac, beta, SE, pval, pval_noadj, converged)."""
    maf, _ = ds_mat_mafmac(ds)
    tsum = [trunc_sum(row) for row in ds]
    res = []
    for b1, b2 in wbeta.T:
        ws = normalize([dbeta(m, b1, b2) for m in maf])
        G = ds_mat_burden(ds, ws, tsum)
        summac = G.sum() * len(ds)
        r = (float("nan"),) * 4 + (False,)
        if summac >= summac_thr and summac > 0:
            r = single(oracle, G)
        res.append((summac,) + r)
    return res


def acatv_unit(oracle, ds, wbeta, acatv_mac, summac_thr):
    """-> (p per weight set, n.single, n.burden as saige_acatv_test_bin reports them, :819-823)."""
    maf, mac = ds_mat_mafmac(ds)
    tsum = [trunc_sum(row) for row in ds]
    ps, counts = [], None
    for b1, b2 in wbeta.T:
        w_pval, pvals, w_burden = [], [], []
        n_burden, summaf = 0, 0.0
        for j in range(len(ds)):
            if mac[j] >= acatv_mac:
                pv = single(oracle, as_f64(ds[j]))[2]
                p = maf[j]
                w_pval.append(dbeta(p, b1, b2) ** 2 * p * (1 - p))
                pvals.append(pv)
                w_burden.append(float("nan"))
            else:
                n_burden += 1
                summaf += maf[j]
                w_burden.append(dbeta(maf[j], b1, b2))
        if n_burden > 0:
            G = ds_mat_burden(ds, normalize(w_burden), tsum)
            summac = G.sum() * len(ds)
            if summac >= summac_thr and summac > 0:
                pv = single(oracle, G)[2]
                if math.isfinite(pv):
                    p = summaf / n_burden
                    w_pval.append(dbeta(p, b1, b2) ** 2 * p * (1 - p))
                    pvals.append(pv)
        if counts is None:
            counts = (len(pvals) - n_burden, n_burden)                # ans[8] = n_single - n_burden, as the reference has it
        ps.append(acat_pval(pvals, w_pval) if pvals else float("nan"))
    return ps, counts[0], counts[1]


def acato_unit(oracle, ds, wbeta, acatv_mac, summac_thr):
    pb = [r[3] for r in burden_unit(oracle, ds, wbeta, summac_thr)]
    pv = acatv_unit(oracle, ds, wbeta, acatv_mac, summac_thr)[0]
    both = []
    for a, b in zip(pb, pv):
        both += [a, b]
    return acat_pval(both, [1.0] * len(both)), pb, pv


class _NumpyDosageBlock:
    def __init__(self, sc, dtype, cap):
        self.sc, self.dtype, self.cap, self.rows = sc, np.dtype(dtype), cap, None
        sc.uploads = getattr(sc, "uploads", 0)

    def load(self, dosage):
        assert dosage.dtype == self.dtype and dosage.shape[0] <= self.cap and dosage.shape[1] == self.sc.n
        self.rows = dosage.copy()
        self.sc.uploads += 1
        ok = np.stack([ok_mask(r) for r in self.rows])
        n = ok.sum(axis=1).astype(np.int32)
        if self.dtype == np.float64:
            z = np.where(ok, self.rows, 0.0)
            return n, z.sum(axis=1), np.floor(z).astype(np.int64).sum(axis=1)
        z = np.where(ok, self.rows, 0).astype(np.int64).sum(axis=1)
        return n, z.astype(np.float64), z

    def scan(self):
        return self.sc.scan_f64(np.stack([as_f64(r) for r in self.rows]))

    def burden(self, grp_ptr, var_idx, flip, w, mw):
        ng, nc = len(grp_ptr) - 1, w.shape[1]
        out = np.zeros((ng * nc, self.sc.n))
        for g in range(ng):
            for e in range(int(grp_ptr[g]), int(grp_ptr[g + 1])):
                row = self.rows[var_idx[e]]
                ok = ok_mask(row)
                if self.dtype == np.float64:
                    x = np.where(ok, row, 0.0)
                    t = 2 - x if flip[e] else x
                else:
                    x = np.where(ok, row, 0).astype(np.int64)
                    t = ((2 - x) if flip[e] else x).astype(np.float64)
                for c in range(nc):
                    if math.isfinite(w[e, c]):
                        out[g * nc + c] += np.where(ok, t * w[e, c], mw[e, c])
        return self.sc.scan_f64(out)

    def close(self):
        self.rows = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class NumpyDsScanner(OracleScanner):
    """``OracleScanner`` plus ``dosage_block``: load / scan / burden of a batch of dosage rows in numpy."""
    last = None

    def __init__(self, sm):
        super().__init__(sm)
        self.uploads = 0
        NumpyDsScanner.last = self

    def dosage_block(self, dtype, max_variants):
        return _NumpyDosageBlock(self, dtype, max_variants)


# ---- cases and checks shared by the CPU and the GPU tests ---------------------------------------------------------
def close(a, c, what):
    """tests/test_aggregate.py::close: 1e-9 relative, NaN patterns equal."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(c)), f"{what}: NaN pattern {a} vs {c}"
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - c[ok]) <= 1e-9 * np.abs(c[ok]) + 1e-300), f"{what}: {a} vs {c}"


def same_dicts(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), f"{what}: column {k}"


def run_drivers(src, mod, units, **kw):
    from saigegds_amd.aggregate import seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaACAT_V, seqAssocGLMM_spaBurden
    b = seqAssocGLMM_spaBurden(src, mod, units, verbose=False, **kw)
    v = seqAssocGLMM_spaACAT_V(src, mod, units, verbose=False, **kw)
    o = seqAssocGLMM_spaACAT_O(src, mod, units, verbose=False, **kw)
    return b, v, o


def check_against_restatement(b, v, o, ds, units, orc, what, spa_pval=0.05, need_spa=True, integer_input=False):
    """ds: the dosage matrix [variant, sample] in the model's sample order.  Every unit of burden, ACAT-V and ACAT-O
    against the restatement; ACAT-O's columns against the stand-alone drivers (test.saige_acta_o); and the cap: at
    least half of the burden rows finite and at least one through the saddlepoint stage (p.norm <= spa_pval)."""
    from saigegds_amd.aggregate import AggrParamBeta as wb
    for k in ("1_1", "1_25"):
        assert np.array_equal(o["pval.b" + k], b["pval.b" + k], equal_nan=True), what
        assert np.array_equal(o["pval.v" + k], v["pval.v" + k], equal_nan=True), what
    n_fin = n_rows = n_spa = 0
    for u, ix in enumerate(units):
        du = ds[np.asarray(ix) - 1]
        rb = burden_unit(orc, du, wb, 3)
        for i, k in enumerate(("b1_1", "b1_25")):
            close([b["summac." + k][u], b["beta." + k][u], b["SE." + k][u], b["pval." + k][u], b["p.norm." + k][u]],
                  rb[i][:5], f"{what}: burden unit {u} {k}")
            assert bool(b["cvg." + k][u]) == bool(rb[i][5]) or math.isnan(rb[i][3])
            n_rows += 1
            n_fin += bool(np.isfinite(rb[i][3]))
            n_spa += bool(np.isfinite(rb[i][4]) and rb[i][4] <= spa_pval)
        pv, n_single, n_burden = acatv_unit(orc, du, wb, 10, 3)
        close([v["pval.v1_1"][u], v["pval.v1_25"][u]], pv, f"{what}: ACAT-V unit {u}")
        assert (int(v["n.single"][u]), int(v["n.burden"][u])) == (n_single, n_burden), f"{what}: unit {u} counts"
        po, _, _ = acato_unit(orc, du, wb, 10, 3)
        close([o["pval"][u]], [po], f"{what}: ACAT-O unit {u}")
        maf, mac = ds_mat_mafmac(du)
        assert b["numvar"][u] == len(ix)
        if integer_input:
            assert b["mac.min"][u] == np.nanmin(mac) and b["mac.max"][u] == np.nanmax(mac), f"{what}: unit {u} mac"
        else:
            close([b["mac.min"][u], b["mac.max"][u]], [np.nanmin(mac), np.nanmax(mac)], f"{what}: unit {u} mac")
        fin = maf[np.isfinite(maf)]
        close([b["maf.avg"][u]], [fin.mean() if fin.size else np.nan], f"{what}: unit {u} maf")
    assert 2 * n_fin >= n_rows, f"{what}: only {n_fin} of {n_rows} burden rows are finite"
    if need_spa:
        assert n_spa >= 1, f"{what}: no burden row went through the saddlepoint stage"


def golden_model():
    import os
    from conftest import GOLDEN, load_null_model
    assert os.path.exists(os.path.join(GOLDEN, "saige_model.npz"))
    return load_null_model("saige_model.npz")


def oracle_for(mod, sample_ids, spa_pval=0.05):
    """Oracle of the model as the aggregate drivers flatten it (thresholds 0 / 0 / 1), samples in the given order."""
    from oracle.oracle import Oracle
    from saigegds_amd.nullmod import init_nullmod
    pos = {str(s): i for i, s in enumerate(mod.sample_id)}
    ii = np.array([pos[str(s)] for s in sample_ids], dtype=np.int64)
    return Oracle(init_nullmod(mod, ii, 0.0, 0.0, 1.0, spa_pval, float(np.nanmean(mod.var_ratio))))


def case_c1():
    """assoc_100snp.gds (dosages in annotation/format/DS, no genotype node), windows of 10 variants."""
    import os
    from conftest import GOLDEN
    from saigegds_amd.gds import GdsFile
    path = os.path.join(GOLDEN, "assoc_100snp.gds")
    g = GdsFile(path)
    ds = g.dosage_real()
    units = [np.arange(s, s + 10) + 1 for s in range(0, 100, 10)]
    return path, ds, [str(s) for s in g.sample_id()], units


def case_c2(seed=20, n_var=240, win=12):
    """Fractional dosages on the k/127 grid from the hard calls of grm1k_10k_snp (noise, clipped to [0, 2], 1 % NaN),
    a few variants with the alt allele the major one, one variant all missing, one monomorphic variant."""
    import os
    from conftest import GOLDEN
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    rng = np.random.default_rng(seed)
    codes = unpack_dosage_2bit(g["packed"][:n_var], 1000).astype(np.float64)
    miss = codes == 3
    x = np.where(miss, 0.0, codes)
    for j in (j for j in (5, 40, 111) if j < n_var):
        x[j] = 2 - x[j]                                   # alt-major
    x = np.clip(x + rng.normal(0, 0.08, x.shape) * (rng.random(x.shape) < 0.3), 0, 2)
    x = np.rint(x * 127) / 127                            # the k/127 grid
    x[miss | (rng.random(x.shape) < 0.01)] = np.nan
    x[17] = np.nan                                        # all missing
    if n_var > 30:
        x[30] = np.where(np.isnan(x[30]), np.nan, 0.0)    # monomorphic
    units = [np.arange(s, min(n_var, s + win)) + 1 for s in range(0, n_var, win)]
    return x, [str(s) for s in g["sample_id"]], units
