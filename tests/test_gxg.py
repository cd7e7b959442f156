"""seqGLMM_GxG_spa (saigegds_amd/gxg.py) on the CPU: the full saddlepoint approximation against the
oracle's restatement of src/SPATest.cpp, the argument checks of R/saige_interaction.r, the interaction
statistic against a dense solve, the options and the result files.  The GRM operator is the CPU oracle
(oracle/grm_oracle.c) on a subset of the grm1k_10k_snp markers."""
import math
import os

import numpy as np
import pytest

from saigegds_amd.assoc import GenotypeSource
from saigegds_amd.gxg import (DosageMatrix, GxGTable, minor_allele_geno, saddle_prob, saige_gxg_snp_bin,
                              seqGLMM_GxG_spa)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GRM_VARIANTS = list(range(1, 10001, 20))       # 500 GRM markers: the oracle's products stay fast


@pytest.fixture(scope="module")
def inputs():
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    src = GenotypeSource(list(g["sample_id"]), packed=g["packed"], variant_id=g["variant_id"])
    data = {"sample.id": ph["sample_id"], "y": ph["y"], "x1": ph["x1"], "x2": ph["x2"]}
    return src, data


def _oracle(p, n):
    from oracle import GrmOracle
    return GrmOracle(p, n)


def _run(inputs, pairs=None, **kw):
    src, data = inputs
    pairs = pairs or {"s1": np.array([2, 3]), "s2": np.array([6, 7])}
    kw.setdefault("variant_id", GRM_VARIANTS)
    kw.setdefault("verbose", False)
    return seqGLMM_GxG_spa("y ~ x1 + x2", data, src, None, pairs, operator_factory=_oracle, **kw)


# ---------------------------------------------------------------------------
# Saddle_Prob


def _spa_case(seed, n=800, rare=False):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.02, 0.6, n)
    if rare:
        g = np.zeros(n)
        g[rng.choice(n, 6, replace=False)] = rng.uniform(0.5, 2.0, 6)
    else:
        g = rng.standard_normal(n) * rng.uniform(0.1, 2.0, n)
    m1 = float(np.sum(mu * g))
    var1 = float(np.sum(mu * (1 - mu) * g * g))
    return mu, g, m1, var1


def _vs_oracle(q, m1, var1, mu, g, cutoff=2.0):
    from oracle import oracle as orc
    p, p_noadj, conv = saddle_prob(q, m1, var1, mu, g, cutoff)
    ref, ref_conv, _ = orc.saddle_prob_fast(q, m1, var1, mu, g, np.arange(mu.size), cutoff)
    assert conv == ref_conv
    assert abs(p - ref) <= 1e-10 * abs(ref), (p, ref)
    assert abs(p_noadj - orc.pchisq1_upper((q - m1) ** 2 / var1)) <= 1e-12 * p_noadj
    return p, p_noadj


def test_saddle_prob_matches_oracle():
    for seed in range(6):
        mu, g, m1, var1 = _spa_case(seed)
        sd = math.sqrt(var1)
        for z in (0.5, -1.5, 2.5, -3.5, 6.0, -9.0):
            p, p_noadj = _vs_oracle(m1 + z * sd, m1, var1, mu, g)
            if abs(z) < 2:
                assert p == p_noadj                 # inside the cutoff: the normal p-value


def test_saddle_prob_root_at_infinity():
    # q >= g_pos: no root (getroot_K1 returns Inf, the tail contributes 0)
    mu, g, m1, var1 = _spa_case(7, rare=True)
    g_pos = float(g[g > 0].sum())
    p, p_noadj = _vs_oracle(g_pos, m1, var1, mu, g)
    assert p == 0.0 < p_noadj               # both tails out of reach (qinv <= g_neg = 0 as well)
    # one tail at infinity, the other a finite saddlepoint
    mu, g, m1, var1 = _spa_case(8, n=300)
    g = -np.abs(g)
    g[:3] = 5.0
    m1, var1 = float(np.sum(mu * g)), float(np.sum(mu * (1 - mu) * g * g))
    g_pos = float(g[g > 0].sum())
    q = g_pos
    assert 2 * m1 - q > float(g[g < 0].sum())
    p, p_noadj = _vs_oracle(q, m1, var1, mu, g)
    assert 0 < p


def test_saddle_prob_cutoff_doubles():
    # a score of bounded support (64 carriers, mu = 0.5): at |q - m1| / sd = 7.8 the saddlepoint
    # p-value is > 1000 x under the normal one, so the cutoff doubles (2 -> 4 -> 8) past 7.8 and the
    # normal p-value is returned
    from saigegds_amd.gxg import _get_saddle_prob, _getroot_k1
    mu, g = np.full(64, 0.5), np.ones(64)
    m1, var1 = float(np.sum(mu * g)), float(np.sum(mu * (1 - mu) * g * g))
    q = m1 + 7.8 * math.sqrt(var1)
    qinv = 2 * m1 - q
    (r1, c1), (r2, c2) = _getroot_k1(64.0, 0.0, mu, g, q), _getroot_k1(64.0, 0.0, mu, g, qinv)
    p_spa = abs(_get_saddle_prob(r1, mu, g, q)) + abs(_get_saddle_prob(r2, mu, g, qinv))
    p, p_noadj = _vs_oracle(q, m1, var1, mu, g)
    assert c1 and c2 and p_noadj / p_spa > 1000
    assert p == p_noadj
    assert saddle_prob(q, m1, var1, mu, g, 16.0)[0] == p_noadj       # (inside the cutoff from the start)
    p8, _ = _vs_oracle(q + 0.3 * math.sqrt(var1), m1, var1, mu, g)   # z = 8.1: past every doubling to 16
    assert p8 >= 0


# ---------------------------------------------------------------------------
# arguments, genotypes


def test_argument_checks(inputs, tmp_path):
    src, data = inputs
    with pytest.raises(ValueError, match="missing values"):
        _run(inputs, {"a": np.array([2.0, np.nan]), "b": np.array([6.0, 7.0])})
    with pytest.raises(ValueError, match="same variant in a pair"):
        _run(inputs, {"a": np.array([2, 3]), "b": np.array([6, 3])})
    with pytest.raises(ValueError, match=r"No variant ID\(s\): 123456, 99999"):
        _run(inputs, {"a": np.array([2, 123456]), "b": np.array([99999, 7])})
    with pytest.raises(NotImplementedError, match="Not implement yet."):
        _run(inputs, trait_type="quantitative")
    with pytest.raises(ValueError, match="Unknown format of the output file"):
        _run(inputs, {"a": [2], "b": [6]}, use_approx_tau=True, model_savefn=str(tmp_path / "out.xlsx"))
    with pytest.raises(ValueError, match="ncol"):
        _run(inputs, {"a": np.array([2, 3])})
    mat = DosageMatrix(np.zeros((3, 2)), ["a", "b", "c"], ["v1", "v2"])
    with pytest.raises(ValueError, match=r"No variant ID\(s\): v3"):
        seqGLMM_GxG_spa("y ~ x1", data, src, mat, {"a": ["v1"], "b": ["v3"]}, operator_factory=_oracle,
                        variant_id=GRM_VARIANTS, verbose=False)


def test_minor_allele_geno():
    g = minor_allele_geno([0, 1, np.nan, 2, 0])
    assert np.allclose(g, [0, 1, 0.75, 2, 0])
    f = minor_allele_geno([2, 2, np.nan, 1, 2])                    # mean 1.75 > 1: flipped after imputing
    assert np.allclose(f, [0, 0, 0.25, 1, 0])
    assert np.allclose(minor_allele_geno([np.nan, np.nan]), [0, 0])   # all missing: af = 0
    assert np.allclose(minor_allele_geno([1, 1, 1, 1]), [1, 1, 1, 1])  # mean exactly 1 stays


# ---------------------------------------------------------------------------
# the interaction statistic against a dense restatement


def test_interaction_statistic_against_dense_solve(inputs):
    from scipy.special import ndtri
    from oracle import GrmOracle
    from saigegds_amd.fitnull import _Fitter, _Param, RRandom, glm_fit
    from saigegds_amd.gds import unpack_dosage_2bit
    from saigegds_amd.gxg import _drop_aliased, _null_model_noK, _qr_design
    src, data = inputs
    packed = np.asarray(src.packed)[::20]
    n = 1000
    op = GrmOracle(packed, n)
    K = np.column_stack([op.crossprod(np.eye(n)[i]) for i in range(n)])
    y = data["y"].astype(np.float64)
    codes = unpack_dosage_2bit(np.asarray(src.packed)[[1, 5]], n).astype(np.float64)
    codes[codes == 3] = np.nan
    g1, g2 = minor_allele_geno(codes[0]), minor_allele_geno(codes[1])
    X = np.column_stack([np.ones(n), data["x1"], data["x2"], g1, g2])
    X1 = _qr_design(X[:, _drop_aliased(X)])
    fit0 = glm_fit(X1, y, "binomial")
    noK = _null_model_noK(X1, y, fit0)
    tau = np.array([1.0, 0.37])
    param = _Param(seed=200, tol=0.02, tolPCG=1e-20, maxiter=20, maxiterPCG=3000, nrun=30, num_marker=1,
                   traceCVcutoff=0.0025, ratioCVcutoff=0.001, verbose=False)
    for batched in (False, True):
        d = saige_gxg_snp_bin(_Fitter(op, X1, y, fit0, param, RRandom(1), batched=batched), fit0, tau, g1 * g2, noK)
        # dense: Sigma = tau0 diag(1/W) + tau1 K, solved directly
        mu = fit0.fitted_values
        W = mu * (1 - mu)
        Sigma = np.diag(tau[0] / W) + tau[1] * K
        G0 = g1 * g2
        G = G0 - noK["XXVX_inv"] @ (noK["XV"] @ G0)
        Si_X, Si_G = np.linalg.solve(Sigma, X1), np.linalg.solve(Sigma, G)
        adj = Si_X @ np.linalg.solve(X1.T @ Si_X, X1.T @ Si_G)
        var1 = G @ Si_G - G @ adj
        beta = ((y - mu) @ G) / var1
        var2 = np.sum(W * G * G)
        m1 = mu @ G
        qt = (y @ G - m1) / math.sqrt(var1) * math.sqrt(var2) + m1
        pval = saddle_prob(qt, m1, var2, mu, G)[0]
        SE = abs(beta / ndtri(pval / 2))
        assert d["n_nonzero"] == int(np.count_nonzero(G0))
        for k, ref in (("beta", beta), ("SE", SE), ("pval", pval)):
            assert abs(d[k] - ref) <= 1e-8 * abs(ref), (k, d[k], ref)
        assert d["tau_G"] == 0.37


# ---------------------------------------------------------------------------
# options and output


def test_columns_approx_tau_and_extra_columns(inputs):
    pairs = {"s1": np.array([2, 3]), "s2": np.array([6, 7]), "note": np.array(["F1", "F2"]),
             "k": np.array([5, 9])}
    r = _run(inputs, pairs, use_approx_tau=True)
    assert isinstance(r, GxGTable)
    assert list(r) == ["id1", "snp1", "maf1", "id2", "snp2", "maf2", "beta", "SE", "n_nonzero", "pval", "p.norm",
                       "converged", "tau_G", "note", "k"]
    assert r["snp1"].tolist() == ["1:2_A_C", "1:3_A_C"]          # GenotypeSource alleles: ref A, alt C
    assert r["note"].tolist() == ["F1", "F2"] and r["k"].tolist() == [5, 9]
    assert r.attrs["tau_G"] == r["tau_G"][0] == r["tau_G"][1] > 0
    assert np.all((r["pval"] > 0) & (r["pval"] <= 1)) and np.all(r["converged"])
    # the same pairs refitted one by one from the approximate tau: no_iteration keeps tau
    r2 = _run(inputs, {"s1": [3], "s2": [7]}, use_approx_tau=True)
    assert r2["beta"][0] == r["beta"][1] and r2.attrs["tau_G"] == r.attrs["tau_G"]


def test_glm_threshold_columns_and_skip(inputs):
    r = _run(inputs, use_approx_tau=True, glm_threshold=True)
    assert list(r)[-2:] == ["p.glm", "p.glm.norm"]
    assert np.all(r["p.glm"] > 0.01)                              # none passes: the GLMM is skipped
    assert np.all(np.isnan(r["pval"])) and np.all(np.isnan(r["p.norm"]))
    assert np.all(r["tau_G"] == 0)                                # the glm pre-screen's tau = (1, 0)
    r1 = _run(inputs, use_approx_tau=True, glm_threshold=1.0)     # all pass: GLMM p-values and the glm columns
    base = _run(inputs, use_approx_tau=True)
    assert np.array_equal(r1["pval"], base["pval"]) and np.array_equal(r1["p.glm"], r["p.glm"])
    assert "p.glm" not in base


def test_matrix_input_and_missing_samples(inputs, capsys):
    src, data = inputs
    from saigegds_amd.gds import unpack_dosage_2bit
    codes = unpack_dosage_2bit(np.asarray(src.packed)[[1, 5]], 1000).astype(np.float64).T
    codes[codes == 3] = np.nan
    sid = list(src.sample_id())
    mat = DosageMatrix(codes[10:], sid[10:], ["rsA", "rsB"])     # 10 samples missing from the matrix
    r = seqGLMM_GxG_spa("y ~ x1 + x2", data, src, mat, {"a": ["rsA"], "b": ["rsB"]}, operator_factory=_oracle,
                        variant_id=GRM_VARIANTS, use_approx_tau=True, verbose=True, verbose_detail=False)
    assert "Missing sample rate in the association GDS file: 0.01%" in capsys.readouterr().out
    assert r["id1"].tolist() == [1] and r["id2"].tolist() == [2]
    assert r["snp1"].tolist() == ["rsA"] and r["snp2"].tolist() == ["rsB"]
    assert np.isfinite(r["beta"][0])


def test_output_files_round_trip(inputs, tmp_path):
    from saigegds_amd import rds
    pairs = {"s1": np.array([2, 3]), "s2": np.array([6, 7]), "note": np.array(["F1", "F2"])}
    r = None
    for ext in ("rds", "RData", "txt", "csv"):
        fn = str(tmp_path / f"gxg.{ext}")
        r = _run(inputs, pairs, use_approx_tau=True, model_savefn=fn)
        if ext == "rds":
            df = rds.read_rds(fn)
            cols = rds.data_frame_columns(df)
            assert list(cols) == list(r)
            assert df.attr["tau_G"][0] == r.attrs["tau_G"]
        elif ext == "RData":
            cols = rds.data_frame_columns(rds.read_rdata(fn)[".x"])
        else:
            sep = "," if ext == "csv" else "\t"
            lines = open(fn).read().splitlines()
            head = [h.strip('"') for h in lines[0].split(sep)]
            assert head == list(r)
            rows = [ln.split(sep) for ln in lines[1:]]
            cols = {h: [row[i].strip('"') for row in rows] for i, h in enumerate(head)}
            if ext == "csv":
                assert lines[1].split(sep)[1] == '"1:2_A_C"'        # write.csv quotes strings
            assert cols["converged"] == ["TRUE", "TRUE"]
            cols = {k: (np.asarray(v, dtype=np.float64) if k not in ("snp1", "snp2", "note", "converged") else v)
                    for k, v in cols.items()}
        for k in ("beta", "SE", "pval", "maf1", "tau_G"):
            np.testing.assert_allclose(np.asarray(cols[k], dtype=np.float64), r[k], rtol=1e-14, atol=0)
        assert [str(v) for v in cols["note"]] == ["F1", "F2"]
        assert [int(v) for v in cols["n_nonzero"]] == r["n_nonzero"].tolist()
