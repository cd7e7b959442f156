"""Leave-one-chromosome-out null models on the CPU: ``seqFitNullGLMM_SPA(loco=True)`` with the oracle's GRM
operator injected (it has no ``pcg_loco``, so the driver builds one operator per chromosome from the markers
outside it), the model file round trip of the ``loco`` entries, and the refusals."""
import os

import numpy as np
import pytest

from saigegds_amd.assoc import GenotypeSource
from saigegds_amd.fitnull import RRandom, _Fitter, _Param, glm_fit, seqFitNullGLMM_SPA
from saigegds_amd.gds import GdsFile
from saigegds_amd.nullmod import NullModel, load_modobj

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GDS = os.path.join(GOLD, "grm1k_10k_snp.gds")
LOCO_KEYS = ("coefficients", "linear_predictors", "fitted_values", "residuals", "cov")


def _data():
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    return {"sample.id": ph["sample_id"], "y": ph["y"], "yy": ph["yy"], "x1": ph["x1"], "x2": ph["x2"]}


def _file_markers():
    """The golden file holds chromosome 1 (9988 variants) and 2 (12): every 8th variant of 1 and all of 2."""
    f = GdsFile(GDS)
    ids, chrom = np.asarray(f.read("variant.id")), np.asarray([str(c) for c in f.read("chromosome")])
    assert sorted(set(chrom)) == ["1", "2"]
    pick = (chrom == "2") | (np.arange(ids.size) % 8 == 0)
    packed, n_all, _ = f.dosage_alt_packed()
    return ids, chrom, pick, np.asarray(packed), n_all


def three_chromosome_source(step=8):
    """The golden genotypes, every ``step``-th variant, relabelled into three chromosomes of unequal size."""
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    packed = np.ascontiguousarray(g["packed"][::step])
    m = packed.shape[0]
    chrom = np.where(np.arange(m) < m // 2, "1", np.where(np.arange(m) < (5 * m) // 6, "2", "X"))
    return GenotypeSource(list(g["sample_id"]), packed=packed, variant_id=g["variant_id"][::step], chromosome=list(chrom),
                          position=g["position"][::step])


@pytest.fixture(scope="module")
def file_fits(tmp_path_factory):
    from oracle.oracle import GrmOracle
    ids, _, pick, _, _ = _file_markers()
    fn = str(tmp_path_factory.mktemp("loco") / "model.rds")
    kw = dict(variant_id=ids[pick], X_transform=False, verbose=False, operator_factory=GrmOracle)
    plain = seqFitNullGLMM_SPA("y ~ x1 + x2", _data(), GDS, **kw)
    loco = seqFitNullGLMM_SPA("y ~ x1 + x2", _data(), GDS, loco=True, model_savefn=fn, **kw)
    return plain, loco, fn


def _by_hand(mod, packed, chrom_of_marker, family, n):
    """get_coeff at the fitted tau, started from the full model, on an operator of the other chromosomes' markers."""
    from oracle.oracle import GrmOracle
    param = _Param(seed=200, tol=0.02, tolPCG=1e-5, maxiter=20, maxiterPCG=500, nrun=30, num_marker=30,
                   traceCVcutoff=0.0025, ratioCVcutoff=0.001, verbose=False)
    fit0 = glm_fit(mod.X1, mod.y, family)
    out = {}
    for ch in dict.fromkeys(chrom_of_marker):
        op = GrmOracle(np.ascontiguousarray(packed[chrom_of_marker != ch]), n)
        out[ch] = _Fitter(op, mod.X1, mod.y, fit0, param, RRandom(200)).get_coeff(mod.tau, mod.coefficients, mod.linear_predictors)
    return out


def _check_entries(mod, want):
    assert list(mod.loco) == list(want)
    for ch, c in want.items():
        e = mod.loco[ch]
        assert sorted(e) == sorted(LOCO_KEYS)
        for key, val in (("coefficients", c["alpha"]), ("linear_predictors", c["eta"]), ("fitted_values", c["mu"]),
                         ("residuals", mod.y - c["mu"]), ("cov", c["cov"])):
            assert np.array_equal(e[key], val), (ch, key)
        assert not np.array_equal(e["fitted_values"], mod.fitted_values), ch     # a different model than the full one


def test_loco_entries_on_the_golden_file(file_fits):
    plain, loco, _ = file_fits
    # the full model is untouched by loco=True
    for k in ("tau", "var_ratio", "fitted_values", "coefficients", "linear_predictors"):
        assert np.array_equal(getattr(plain, k), getattr(loco, k)), k
    assert plain.loco == {} and loco.tau[1] > 0
    ids, chrom, pick, packed, n_all = _file_markers()
    assert np.array_equal(np.asarray(loco.variant_id), ids[pick]) and n_all == len(loco.sample_id)
    _check_entries(loco, _by_hand(loco, packed[pick], chrom[pick], "binomial", n_all))
    assert all(s["steps"] >= 1 and len(s["pcg_iters"]) == s["steps"] for s in loco.loco_steps.values())


def test_loco_entries_on_three_chromosomes_quantitative():
    from oracle.oracle import GrmOracle
    src = three_chromosome_source()
    kw = dict(trait_type="quantitative", X_transform=False, verbose=False, operator_factory=GrmOracle)
    plain = seqFitNullGLMM_SPA("yy ~ x1 + x2", _data(), src, **kw)
    loco = seqFitNullGLMM_SPA("yy ~ x1 + x2", _data(), src, loco=True, **kw)
    for k in ("tau", "var_ratio", "fitted_values"):
        assert np.array_equal(getattr(plain, k), getattr(loco, k)), k
    keep = np.isin(src.variant_id, np.asarray(loco.variant_id))
    assert list(loco.loco) == ["1", "2", "X"]
    _check_entries(loco, _by_hand(loco, src.packed[keep], np.asarray(src.chromosome)[keep], "gaussian", len(loco.sample_id)))


def test_model_file_round_trip(file_fits, tmp_path):
    from saigegds_amd.results import save_model
    plain, loco, fn = file_fits
    back = load_modobj(fn)
    assert list(back.loco) == list(loco.loco)
    for ch, e in loco.loco.items():
        for k in LOCO_KEYS:
            assert np.array_equal(back.loco[ch][k], np.asarray(e[k])) and back.loco[ch][k].shape == np.shape(e[k]), (ch, k)
    for k in ("tau", "fitted_values", "var_ratio", "y", "V", "X1", "XV", "XXVX_inv", "coefficients"):
        assert np.array_equal(np.asarray(getattr(back, k)), np.asarray(getattr(loco, k))), k
    alt = back.for_chromosome("2")
    assert np.array_equal(alt.fitted_values, loco.loco["2"]["fitted_values"]) and alt.loco == {}
    assert np.array_equal(alt.y, back.y) and np.array_equal(alt.XXVX_inv, back.XXVX_inv)
    # a model file without the entries loads as before
    fn2 = str(tmp_path / "plain.RData")
    save_model(plain, fn2)
    assert load_modobj(fn2).loco == {}
    assert load_modobj(os.path.join(GOLD, "saige_model_quant.rds")).loco == {}


def test_chromosome_count_errors():
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    packed = np.ascontiguousarray(g["packed"][:130])
    sid = list(g["sample_id"])

    def refuse(chrom, match):
        src = GenotypeSource(sid, packed=packed, chromosome=chrom)
        with pytest.raises(ValueError, match=match):
            seqFitNullGLMM_SPA("y ~ x1", _data(), src, variant_id=np.arange(1, 131), loco=True, verbose=False,
                               operator_factory=lambda p, n: pytest.fail("the fit started"))

    refuse(["7"] * 130, "more than one chromosome.*chromosome '7'")
    refuse([str(i % 65) for i in range(130)], "at most 64 chromosomes.*65")


def test_other_drivers_refuse_a_loco_model():
    from saigegds_amd import (seqAssocGLMM_SPA_cond, seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaACAT_V, seqAssocGLMM_spaBurden,
                              seqAssocGLMM_spaSKAT)
    z = np.load(os.path.join(GOLD, "saige_model.npz"))
    mod = NullModel(trait_type="binary", tau=z["tau"], fitted_values=z["fitted_values"], sample_id=list(z["sample_id"]),
                    var_ratio=z["var_ratio"], y=z["y"], V=z["V"], X1=z["X1"], XV=z["XV"], XXVX_inv=z["XXVX_inv"],
                    loco={"1": {"fitted_values": z["fitted_values"]}})
    src = three_chromosome_source(step=100)
    units = [np.arange(1, 11)]
    msgs = set()
    for f in (seqAssocGLMM_spaBurden, seqAssocGLMM_spaACAT_V, seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaSKAT):
        with pytest.raises(NotImplementedError, match="leave-one-chromosome-out") as ei:
            f(src, mod, units, verbose=False)
        msgs.add(str(ei.value).split(":", 1)[1])
    with pytest.raises(NotImplementedError, match="leave-one-chromosome-out") as ei:
        seqAssocGLMM_SPA_cond(src, mod, [1], verbose=False)
    msgs.add(str(ei.value).split(":", 1)[1])
    assert len(msgs) == 1                            # one shared message
