"""SKAT on the host: the mixture p-value ``pchisq_mix`` against the same saddlepoint formula in 40-digit mpmath, and
the driver ``seqAssocGLMM_spaSKAT`` with an injected scanner (scan: the CPU oracle; skat_2bit: tests/skat_ref.py in
double), as tests/test_aggregate.py runs the other aggregate drivers without a GPU."""
import math
import os

import numpy as np
import pytest

import skat_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
P_TARGETS = (0.9, 0.5, 0.1, 1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 1e-12)
_cache = {}


def golden_phi_lambda():
    """Eigenvalues of a Phi of skat_ref: 40 variants of grm1k_10k_snp.npz with the golden binary model."""
    if "lam" not in _cache:
        from conftest import scan_model
        from saigegds_amd.gds import unpack_dosage_2bit
        g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
        sm = scan_model("saige_model.npz", mac=0.0, maf=0.0, missing=1.0)
        packed = g["packed"][:40]
        _, cov = R.skat_ref(sm, packed, [0, 40], np.arange(40), R.tables(unpack_dosage_2bit(packed, 1000)))
        _cache["lam"] = np.linalg.eigvalsh(cov[0].astype(np.float64))
    return _cache["lam"]


def lambda_sets():
    return {"equal": np.ones(4), "geometric": 0.5 ** np.arange(30), "dominant": np.array([1.0] + [1e-3] * 50),
            "golden Phi": golden_phi_lambda()}


def mp_saddle(q, lam):
    """The formula of pchisq_mix's docstring, written down plainly at 40 digits, root by bisection."""
    import mpmath as mp
    with mp.workdps(40):
        lam = [mp.mpf(float(x)) for x in lam]
        q = mp.mpf(float(q))
        lmax = max(lam)
        k1 = lambda t: sum(x / (1 - 2 * t * x) for x in lam)                      # noqa: E731
        if q > sum(lam):
            lo, hi = mp.mpf(0), (1 - lmax / q) / (2 * lmax)
        else:
            lo, hi = -mp.mpf(len(lam)) / (2 * q), mp.mpf(0)
        for _ in range(150):
            mid = (lo + hi) / 2
            if k1(mid) > q:
                hi = mid
            else:
                lo = mid
        t = (lo + hi) / 2
        K = -sum(mp.log(1 - 2 * t * x) for x in lam) / 2
        k2 = 2 * sum(x * x / (1 - 2 * t * x) ** 2 for x in lam)
        w = mp.sign(t) * mp.sqrt(2 * (t * q - K))
        v = t * mp.sqrt(k2)
        return float(mp.ncdf(-(w + mp.log(v / w) / w)))


def q_at(p, lam):
    """q with pchisq_mix(q, lam) ~ p (only picks the test points)."""
    from scipy.optimize import brentq
    from saigegds_amd.skat import pchisq_mix
    hi = float(np.sum(lam))
    while pchisq_mix(hi, lam) > p:
        hi *= 2
    return brentq(lambda x: math.log(pchisq_mix(x, lam)) - math.log(p), 1e-12 * hi, hi, xtol=1e-14 * hi, rtol=1e-12)


@pytest.mark.parametrize("name", ["equal", "geometric", "dominant", "golden Phi"])
def test_pchisq_mix_equals_the_formula_in_mpmath(name):
    from saigegds_amd.skat import LAMBDA_DROP, pchisq_mix
    lam = lambda_sets()[name]
    kept = lam[lam > LAMBDA_DROP * lam.max()]
    assert kept.size > 1
    for p in P_TARGETS:
        q = q_at(p, lam)
        got, ref = pchisq_mix(q, lam), mp_saddle(q, kept)
        print(f"{name}: p target {p:g}, q = {q:.6g}: {got:.15e} against {ref:.15e}, rel {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= 1e-10 * ref, (name, p)
        assert 0.5 * p < got < 2 * p


def test_one_eigenvalue_is_exact():
    from scipy.special import chdtrc
    from saigegds_amd.skat import pchisq_mix
    for q in (1e-3, 0.7, 2.5, 40.0, 300.0):
        assert pchisq_mix(q, [2.5]) == chdtrc(1.0, q / 2.5)
        assert pchisq_mix(q, [2.5, 2.0e-10, 0.0]) == chdtrc(1.0, q / 2.5)      # at or below 1e-10 of the largest: dropped


@pytest.mark.parametrize("name", ["equal", "geometric", "dominant", "golden Phi"])
def test_monotone_and_continuous_through_the_mean(name):
    from saigegds_amd.skat import pchisq_mix
    lam = lambda_sets()[name]
    mean, sd = lam.sum(), math.sqrt(2 * np.sum(lam * lam))
    qs = np.linspace(mean - 3 * sd, mean + 3 * sd, 2001)
    p = np.array([pchisq_mix(q, lam) for q in qs])
    assert np.all(np.isfinite(p)) and np.all((p > 0) & (p <= 1))
    step = p[:-1] - p[1:]
    k = int(np.argmax(step / p[:-1]))
    print(name, "largest step / p", step[k] / p[k], "at q", qs[k], "p at the mean", p[1000])
    assert np.all(step >= 0), "not non-increasing"
    # The step bound holds where the distribution itself moves by less than 1 % of p per grid step.  The "dominant"
    # set is a chi-square of ONE degree of freedom shifted by the 50 small terms (their sum 0.05 +- 0.01): its density
    # is singular at the shift, p falls like sqrt(q - 0.05) there, and the grid's 0.0042 is a true step of 2-5 % for
    # q < 0.1.  That is the distribution, not the formula's switch at the mean (q = 1.05), so for this set the bound
    # is asserted from half a standard deviation below the mean on.
    where = qs[:-1] >= mean - 0.5 * sd if name == "dominant" else np.ones(2000, dtype=bool)
    assert np.all(step[where] <= 0.01 * p[:-1][where]), "a step above 1 % of p"
    assert qs[1000] == pytest.approx(mean, rel=1e-15) and 0.3 < p[1000] < 0.5


def test_q_at_or_below_zero_and_empty_lambda():
    from saigegds_amd.skat import pchisq_mix
    assert pchisq_mix(0.0, [1.0, 2.0]) == 1.0 and pchisq_mix(-3.0, [1.0, 2.0]) == 1.0 and pchisq_mix(0.0, [1.0]) == 1.0
    assert math.isnan(pchisq_mix(1.0, [])) and math.isnan(pchisq_mix(1.0, np.zeros(0)))


# ---- the driver, no GPU -----------------------------------------------------------------------------------------

def ref_scanner_factory():
    """Scanner stand-in: the oracle's scan, skat_2bit = skat_ref in double; counts the skat_2bit calls."""
    from oracle.oracle import OracleScanner

    class RefScanner(OracleScanner):
        calls = 0

        def __init__(self, sm):
            OracleScanner.__init__(self, sm)
            self._sm = sm

        def skat_2bit(self, packed, unit_ptr, var_idx, lut):
            RefScanner.calls += 1
            return R.skat_ref(self._sm, packed, unit_ptr, var_idx, lut, dtype=np.float64)
    return RefScanner


def driver_case(trait):
    """200 golden variants + 3 monomorphic rows + 1 row without a genotype; units incl. an empty and a monomorphic one."""
    from conftest import load_null_model
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:200], 1000)
    extra = np.zeros((4, 1000), dtype=np.uint8)
    extra[1] = 2
    extra[2, ::50] = 3
    extra[3] = 3
    codes = np.concatenate([codes, extra])
    mod = load_null_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz")
    src = GenotypeSource([str(s) for s in g["sample_id"]], packed=pack_dosage_2bit(codes))
    units = [np.arange(1, 41), np.arange(41, 81), np.zeros(0, dtype=np.int64), np.array([201, 202, 203, 204]),
             np.concatenate([np.arange(81, 201), [201, 204]])]
    return src, mod, units, codes


def expected(sm, codes, units, wbeta, adjust=True):
    """Per unit and weight set (n.var, Q, pval): the issue's steps written out on the oracle's table and skat_ref."""
    from oracle.oracle import Oracle
    from scipy.special import chdtri
    from scipy.stats import beta
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.skat import pchisq_mix
    packed = pack_dosage_2bit(codes)
    out, valid = Oracle(sm).scan_2bit(packed)
    ok = codes != 3
    n, s = ok.sum(axis=1), np.where(ok, codes, 0).sum(axis=1)
    mac = np.minimum(s, 2 * n - s)
    with np.errstate(invalid="ignore", divide="ignore"):
        maf = np.minimum(s / (2 * n), 1 - s / (2 * n))
    lut = R.tables(codes)
    res, n_adj = [], 0
    for ix in units:
        r = np.array([v - 1 for v in ix if valid[v - 1] and mac[v - 1] > 0], dtype=np.int64)
        row = [r.size]
        if r.size:
            S, cov = R.skat_ref(sm, packed, [0, r.size], r, lut[r], dtype=np.float64)
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
def test_driver_with_reference_scanner(trait, tmp_path):
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.aggregate import AggrParamBeta
    from saigegds_amd.nullmod import init_nullmod
    from saigegds_amd.rds import read_rdata
    src, mod, units, codes = driver_case(trait)
    fac = ref_scanner_factory()
    fn = str(tmp_path / "skat.RData")
    ans = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=fac, res_savefn=fn)
    assert fac.calls == 1                                           # one skat_2bit call for all units
    for c in ("numvar", "maf.avg", "mac.max", "n.var", "Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25"):
        assert c in ans, c
    assert "Q" not in ans and "pval" not in ans
    assert list(ans["numvar"]) == [40, 40, 0, 4, 122]
    sm = init_nullmod(mod, np.arange(1000), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    exp, n_adj = expected(sm, codes, units, AggrParamBeta)
    assert list(ans["n.var"]) == list(exp[:, 0].astype(int)) and ans["n.var"][2] == 0 and ans["n.var"][3] == 0
    assert ans["n.var"][4] == exp[4, 0] <= 120 and ans["n.var"][0] > 20
    for k, c in enumerate(("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25")):
        close(ans[c], exp[:, 1 + k], 1e-12, f"{trait} {c}")
        assert np.isnan(ans[c][2]) and np.isnan(ans[c][3]) and np.isfinite(ans[c][[0, 1, 4]]).all()
        assert np.all((ans[c][[0, 1, 4]] > 0))
    if trait == "binary":
        # the adjustment is applied where stated -- and only there: leaving it out moves exactly the units that hold
        # an adjusted variant
        assert n_adj >= 2
        plain, _ = expected(sm, codes, units, AggrParamBeta, adjust=False)
        moved = [u for u in (0, 1, 4) if abs(plain[u, 2] - exp[u, 2]) > 1e-9 * exp[u, 2]]
        assert moved, "no unit with an SPA-adjusted variant"
        assert np.array_equal(plain[:, 1], exp[:, 1], equal_nan=True)         # Q itself is not adjusted
    # one weight set: no suffix
    one = seqAssocGLMM_spaSKAT(src, mod, units, wbeta=[1, 25], verbose=False, scanner_factory=fac)
    assert "Q" in one and "pval" in one and "Q.b1_25" not in one
    close(one["pval"], ans["pval.b1_25"], 1e-15, "one weight set")
    # round trip through the result file
    back = next(iter(read_rdata(fn).values()))
    for c in ("n.var", "Q.b1_1", "pval.b1_25"):
        assert np.array_equal(np.asarray(back[c], dtype=np.float64), np.asarray(ans[c], dtype=np.float64), equal_nan=True), c


def test_driver_refuses_dosage_input():
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    src, mod, units, codes = driver_case("binary")
    with pytest.raises(NotImplementedError, match="SKAT on dosage input is not implemented."):
        seqAssocGLMM_spaSKAT(src, mod, units, dsnode="annotation/format/DS", verbose=False, scanner_factory=ref_scanner_factory())
    frac = GenotypeSource(src.sample_id(), dosage=np.where(codes == 3, np.nan, codes * 0.5))
    with pytest.raises(NotImplementedError, match="SKAT on dosage input is not implemented."):
        from aggregate_ds_ref import NumpyDsScanner
        seqAssocGLMM_spaSKAT(frac, mod, units[:2], verbose=False, scanner_factory=NumpyDsScanner)
