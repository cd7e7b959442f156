"""seqAssocGLMM_SPA(firth_pval=) on the device: the golden file and model against the long-double reference of
tests/firth_ref.py on the flagged rows (what the CPU stand-in run of tests/test_firth_driver.py returns), the scan's own
columns bit for bit against the run without the argument, both decode routes, and a LOCO model."""
import os
from dataclasses import replace

import numpy as np
import pytest

import firth_ref as R
from conftest import GOLDEN, REL_TOL, load_null_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]
GDS = os.path.join(GOLDEN, "grm1k_10k_snp.gds")
TODAY = ["AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def _close(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    print(f"{what}: off by {float(err.max()):.3g} relative at worst over {int(ok.sum())} rows")
    assert np.all(err <= REL_TOL), what


def _reference(ans, packed, variant_id, sm):
    """beta.firth / SE.firth / cvg.firth of a result by the reference: the flagged rows' 2-bit rows and AF column."""
    from saigegds_amd import firth
    flagged = ans["pval"] <= 0.05
    rows = np.flatnonzero(np.isin(variant_id, np.asarray(ans["id"])[flagged]))
    lut, flip = firth.firth_tables(ans["AF.alt"][flagged])
    ref = R.firth_ref(sm, packed[rows], lut)
    beta, se, cvg = np.full(flagged.size, np.nan), np.full(flagged.size, np.nan), np.zeros(flagged.size, dtype=bool)
    beta[flagged], se[flagged], cvg[flagged] = np.where(flip, -ref[:, 0], ref[:, 0]), ref[:, 1], ref[:, 3] == 1
    return beta, se, cvg


@pytest.fixture(scope="module")
def golden():
    """The plain run of the golden file, made once, and the reference columns for it."""
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    from saigegds_amd.gds import GdsFile
    from saigegds_amd.nullmod import init_nullmod
    mod = load_null_model("saige_model.npz")
    plain = seqAssocGLMM_SPA(GDS, mod, mac=4, verbose=False)
    g = GdsFile(GDS)
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    assert [str(s) for s in g.sample_id()] == [str(s) for s in mod.sample_id]
    return mod, plain, _reference(plain, g.dosage_alt_packed()[0], np.asarray(g.read("variant.id")), sm)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_golden_file(golden, mode, monkeypatch):
    from saigegds_amd import assoc
    mod, plain, (beta, se, cvg) = golden
    monkeypatch.setattr(assoc, "GENOTYPE_DECODE", mode)
    got = assoc.seqAssocGLMM_SPA(GDS, mod, mac=4, verbose=False, firth_pval=0.05)
    assert list(got) == list(plain) + ["beta.firth", "SE.firth", "cvg.firth"]
    for k in plain:                                          # every scan column bit for bit
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    flagged = got["pval"] <= 0.05
    assert flagged.sum() > 100
    assert np.array_equal(got["cvg.firth"], cvg) and cvg[flagged].all() and not cvg[~flagged].any()
    _close(got["beta.firth"], beta, f"{mode}: beta.firth")
    _close(got["SE.firth"], se, f"{mode}: SE.firth")
    # the bias the column is there for: the Firth estimate is finite everywhere and differs from the one-step beta
    assert np.all(np.isfinite(got["beta.firth"][flagged])) and not np.allclose(got["beta.firth"][flagged], got["beta"][flagged])


def test_in_memory_source_equals_the_file(golden):
    from saigegds_amd.assoc import GenotypeSource, seqAssocGLMM_SPA
    mod, plain, (beta, se, cvg) = golden
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    src = GenotypeSource([str(s) for s in g["sample_id"]], packed=g["packed"], variant_id=g["variant_id"], position=g["position"])
    got = seqAssocGLMM_SPA(src, mod, mac=4, verbose=False, firth_pval=0.05)
    assert np.array_equal(got["pval"], plain["pval"]) and np.array_equal(got["cvg.firth"], cvg)
    _close(got["beta.firth"], beta, "in memory: beta.firth")
    _close(got["SE.firth"], se, "in memory: SE.firth")


def test_loco_rows_use_their_chromosomes_mu():
    from saigegds_amd import firth
    from saigegds_amd.assoc import match_samples, seqAssocGLMM_SPA
    from saigegds_amd.nullmod import init_nullmod
    from test_gpu_loco_scan import _scan_inputs
    mod, loco, chrom, source = _scan_inputs()
    src = source(np.arange(len(chrom)))
    plain = seqAssocGLMM_SPA(src, replace(mod, loco=loco), mac=4, verbose=False)
    got = seqAssocGLMM_SPA(src, replace(mod, loco=loco), mac=4, verbose=False, firth_pval=0.2)
    for k in plain:
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    ii = match_samples(src, mod)[2]
    flagged = got["pval"] <= 0.2
    chr_of = np.asarray(got["chr"])
    seen = 0
    for ch in ("1", "2", "X"):
        m_run = replace(mod, fitted_values=loco[ch]["fitted_values"]) if ch in loco else mod
        sm = init_nullmod(m_run, ii, float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
        pick = flagged & (chr_of == ch)
        assert pick.any()
        rows = np.flatnonzero(np.isin(src.variant_id, np.asarray(got["id"])[pick]))
        lut, flip = firth.firth_tables(got["AF.alt"][pick])
        ref = R.firth_ref(sm, src.packed[rows], lut)
        _close(got["beta.firth"][pick], np.where(flip, -ref[:, 0], ref[:, 0]), f"chromosome {ch}: beta.firth")
        _close(got["SE.firth"][pick], ref[:, 1], f"chromosome {ch}: SE.firth")
        if ch in loco:                                        # ... and not the full model's: that gives another root
            sm0 = init_nullmod(mod, ii, float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
            other = R.firth_ref(sm0, src.packed[rows], lut)
            assert np.max(np.abs(other[:, 0] - ref[:, 0]) / np.abs(ref[:, 0])) > 1e-6
        seen += int(pick.sum())
    assert seen == int(flagged.sum()) == int(got["cvg.firth"].sum())
    assert np.isnan(got["beta.firth"][~flagged]).all()
