"""SKAT on dosage input without a GPU: ``seqAssocGLMM_spaSKAT`` with an injected scanner whose dosage block has a
``skat`` method in numpy (tests/skat_ds_ref.py), against the steps written out on the oracle's dosage scan and the
reference; the tie to the 2-bit driver on hard calls; batching; the C ABI's declaration and binding."""
import math
import os
import re

import numpy as np
import pytest

import skat_ds_ref as D

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fractional_case(n_var=200, seed=31):
    """Fractional float64 dosages from the hard calls of grm1k_10k_snp: in 30 % of the genotypes the call is mixed with
    the variant's expected dosage 2 af (the lower af, the closer it stays to the call); 1 % NaN; rows 5, 40, 111
    alt-major; row 17 all missing; row 30 monomorphic.  Units: three windows, an empty unit, a unit of the all-missing
    and the monomorphic row alone, a large unit that holds both."""
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    rng = np.random.default_rng(seed)
    codes = unpack_dosage_2bit(g["packed"][:n_var], 1000).astype(np.float64)
    miss = codes == 3
    x = np.where(miss, 0.0, codes)
    for j in (j for j in (5, 40, 111) if j < n_var):
        x[j] = 2 - x[j]
    af = x.sum(axis=1) / (2 * (~miss).sum(axis=1))
    lam = rng.random(x.shape) * np.sqrt(np.minimum(af, 1 - af))[:, None] * (rng.random(x.shape) < 0.3)
    x = (1 - lam) * x + lam * 2 * af[:, None]
    x[miss | (rng.random(x.shape) < 0.01)] = np.nan
    x[17] = np.nan
    x[30] = np.where(np.isnan(x[30]), np.nan, 0.0)
    units = [np.arange(1, 41), np.arange(41, 81), np.zeros(0, dtype=np.int64), np.array([18, 31]),
             np.arange(81, 121), np.concatenate([np.arange(121, n_var + 1), [18, 31]])]
    return x, [str(s) for s in g["sample_id"]], units


def _model(trait):
    from conftest import load_null_model
    return load_null_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz")


def _flat(mod):
    from saigegds_amd.nullmod import init_nullmod
    return init_nullmod(mod, np.arange(1000), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))


def expected(sm, ds, units, wbeta, adjust=True):
    """Per unit and weight set (n.var, Q, pval): the driver's steps written out on the oracle's dosage scan and
    skat_ds_ref in double, unit by unit."""
    from oracle.oracle import Oracle
    from scipy.special import chdtri
    from scipy.stats import beta
    from saigegds_amd.skat import pchisq_mix
    out, valid = Oracle(sm).scan_f64(ds)
    ok = np.isfinite(ds)
    n, s = ok.sum(axis=1).astype(np.float64), np.where(ok, ds, 0.0).sum(axis=1)
    mac = np.minimum(s, 2 * n - s)
    with np.errstate(invalid="ignore", divide="ignore"):
        maf = np.minimum(s / (2 * n), 1 - s / (2 * n))
    flip, mean = D.flip_mean(ds)
    res, n_adj = [], 0
    for ix in units:
        r = np.array([v - 1 for v in ix if valid[v - 1] and mac[v - 1] > 0], dtype=np.int64)
        row = [r.size]
        if r.size:
            S, cov = D.skat_ds_ref(sm, ds, [0, r.size], r, flip[r], mean[r], dtype=np.float64)
            phi = cov[0]
            if not sm.quant and adjust:
                for k, j in enumerate(r):
                    pv, pn, cvg = out[j, 5], out[j, 6], out[j, 7]
                    if pn <= sm.spa_pval and cvg != 0 and pv > 0 and pv != pn and S[k] != 0:
                        d = S[k] ** 2 / (phi[k, k] * chdtri(1.0, pv))
                        phi[k, :] *= math.sqrt(d)
                        phi[:, k] *= math.sqrt(d)
                        n_adj += 1
        for a, b in np.asarray(wbeta).reshape(2, -1).T:
            if r.size == 0:
                row += [float("nan"), float("nan")]
                continue
            w = beta.pdf(maf[r], a, b)
            q = float(np.sum(w * w * S * S))
            row += [q, pchisq_mix(q, np.linalg.eigvalsh(phi * w[:, None] * w[None, :]))]
        res.append(row)
    return np.array(res, dtype=np.float64), n_adj


def close(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    k = ~np.isnan(a)
    assert np.all(np.abs(a[k] - b[k]) <= tol * np.abs(b[k])), (what, a, b)


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_fractional_dosages_against_the_steps_written_out(trait):
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.aggregate import AggrParamBeta
    from saigegds_amd.assoc import GenotypeSource
    ds, sid, units = fractional_case()
    mod = _model(trait)
    ans = seqAssocGLMM_spaSKAT(GenotypeSource(sid, dosage=ds), mod, units, verbose=False,
                               scanner_factory=D.NumpySkatDsScanner)
    sc = D.NumpySkatDsScanner.last
    assert sc.uploads == 1 and sc.skat_calls == 1                  # one batch: one upload, one skat call for all units
    for c in ("numvar", "maf.avg", "mac.max", "n.var", "Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25"):
        assert c in ans, c
    assert "Q" not in ans and "pval" not in ans
    assert list(ans["numvar"]) == [40, 40, 0, 2, 40, 82]
    sm = _flat(mod)
    exp, n_adj = expected(sm, ds, units, AggrParamBeta)
    assert list(ans["n.var"]) == list(exp[:, 0].astype(int)) and ans["n.var"][2] == 0 and ans["n.var"][3] == 0
    assert ans["n.var"][5] == exp[5, 0] <= 80 and ans["n.var"][0] > 20
    for k, c in enumerate(("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25")):
        close(ans[c], exp[:, 1 + k], 1e-12, f"{trait} {c}")
        assert np.isnan(ans[c][2]) and np.isnan(ans[c][3]) and np.isfinite(ans[c][[0, 1, 4, 5]]).all()
        assert np.all(ans[c][[0, 1, 4, 5]] > 0)
    if trait == "binary":
        assert n_adj >= 2
        plain, _ = expected(sm, ds, units, AggrParamBeta, adjust=False)
        moved = [u for u in (0, 1, 4, 5) if abs(plain[u, 2] - exp[u, 2]) > 1e-9 * exp[u, 2]]
        assert moved, "no unit with an SPA-adjusted variant"
        assert np.array_equal(plain[:, 1], exp[:, 1], equal_nan=True)         # Q itself is not adjusted


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_hard_calls_as_float64_equal_the_2bit_driver(trait):
    """A float64 matrix is never rerouted to 2-bit: the same hard calls as float64 (NaN = missing) take the dosage
    flow and give what the 2-bit driver gives on the packed codes."""
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    from test_skat import driver_case, ref_scanner_factory
    src, mod, units, codes = driver_case(trait)
    ref = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=ref_scanner_factory())
    ds = np.where(codes == 3, np.nan, codes.astype(np.float64))
    got = seqAssocGLMM_spaSKAT(GenotypeSource(src.sample_id(), dosage=ds), mod, units, verbose=False,
                               scanner_factory=D.NumpySkatDsScanner)
    assert D.NumpySkatDsScanner.last.skat_calls == 1               # the dosage flow, not skat_2bit
    assert list(got.keys()) == list(ref.keys())
    assert np.array_equal(got["n.var"], ref["n.var"]) and np.array_equal(got["numvar"], ref["numvar"])
    assert got["n.var"][0] > 20 and got["n.var"][2] == 0 and got["n.var"][3] == 0
    for c in ("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25"):
        close(got[c], ref[c], 1e-9, f"{trait} {c}")
        assert np.isfinite(got[c][[0, 1, 4]]).all()


def test_batches_equal_one_batch():
    """Sliding windows of 12 variants, step 8 (units share variants across batch borders) in batches of at most 30
    resident rows against the one-batch run: exactly equal."""
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    ds, sid, _ = fractional_case(n_var=100)
    units = [np.arange(s, s + 12) + 1 for s in range(0, 88, 8)]
    mod = _model("binary")
    src = GenotypeSource(sid, dosage=ds)
    one = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=D.NumpySkatDsScanner)
    assert D.NumpySkatDsScanner.last.uploads == 1
    many = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=D.NumpySkatDsScanner, ds_budget=30 * 8000)
    sc = D.NumpySkatDsScanner.last
    assert sc.uploads >= 3 and sc.skat_calls == sc.uploads
    assert list(one) == list(many)
    for k in one:
        assert np.array_equal(np.asarray(one[k]), np.asarray(many[k]), equal_nan=True), k
    assert np.isfinite(one["pval.b1_25"]).all()


def test_abi_declared_and_bound():
    from saigegds_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "saigehip.h")).read()
    assert re.search(r"\bint\s+sgx_ds_block_skat\s*\(\s*sgx_handle\s*\*h,\s*const\s+sgx_dsblock\s*\*b,", hdr)
    assert "sgx_ds_block_skat" in _lib.EXPORTS
    assert callable(getattr(_lib.DosageBlock, "skat", None))
