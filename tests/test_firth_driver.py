"""seqAssocGLMM_SPA(firth_pval=) and firth_pass on the CPU: the golden genotypes and model through the stand-in scanner of
tests/firth_ref.py (the scan oracle and the long-double Firth reference).  No GPU."""
import os
from dataclasses import replace

import numpy as np
import pytest

import firth_ref as R
from conftest import GOLDEN, load_null_model

M = 1500          # variants of the golden set the driver runs see
TODAY = ["id", "chr", "pos", "ref", "alt", "AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged"]


def _source(m=M):
    """The first m golden variants; every 7th row is turned alt-major (codes 0 and 2 swapped)."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    sid = [str(s) for s in g["sample_id"]]
    codes = unpack_dosage_2bit(g["packed"][:m], len(sid))
    codes[::7] = np.array([2, 1, 0, 3], dtype=np.uint8)[codes[::7]]
    return GenotypeSource(sid, packed=pack_dosage_2bit(codes), variant_id=g["variant_id"][:m], position=g["position"][:m])


@pytest.fixture()
def on_cpu(monkeypatch):
    """The driver with the stand-in for the device: one visible device, RefScanner for Scanner."""
    from saigegds_amd import _lib
    real = _lib.load()

    class OneDevice:
        def __getattr__(self, name):
            return getattr(real, name)

        def sgx_device_count(self):
            return 1

    monkeypatch.setattr(_lib, "load", OneDevice)
    monkeypatch.setattr(_lib, "Scanner", R.RefScanner)
    monkeypatch.setattr(R.RefScanner, "calls", [])
    return R.RefScanner.calls


@pytest.fixture(scope="module")
def runs():
    return {}


def _run(runs, key, **kw):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    if key not in runs:
        runs[key] = seqAssocGLMM_SPA(_source(), load_null_model("saige_model.npz"), mac=4, verbose=False, **kw)
    return runs[key]


def test_none_changes_nothing(on_cpu, runs):
    plain = _run(runs, "plain")
    none = _run(runs, "none", firth_pval=None, firth_maxit=7)
    assert list(plain) == list(none) == TODAY
    for k in TODAY:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(none[k])), k
    assert on_cpu == []                                        # no Firth call was made


def test_columns_on_the_flagged_rows(on_cpu, runs, capsys):
    from saigegds_amd import firth
    from saigegds_amd.nullmod import init_nullmod
    plain, got = _run(runs, "plain"), _run(runs, "firth", firth_pval=0.05)
    assert list(got) == TODAY + ["beta.firth", "SE.firth", "cvg.firth"]
    for k in TODAY:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(got[k])), k
    flagged = got["pval"] <= 0.05
    assert 20 < flagged.sum() < flagged.size
    assert np.isnan(got["beta.firth"][~flagged]).all() and np.isnan(got["SE.firth"][~flagged]).all()
    assert got["cvg.firth"].dtype == bool and not got["cvg.firth"][~flagged].any() and got["cvg.firth"][flagged].all()

    # the reference on those rows, straight from the packed rows and the AF column
    mod, src = load_null_model("saige_model.npz"), _source()
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    rows = np.flatnonzero(np.isin(src.variant_id, got["id"][flagged]))
    af = got["AF.alt"][flagged]
    lut, flip = firth.firth_tables(af)
    assert flip.any() and not flip.all()                       # alt-major rows are among the flagged ones
    assert np.array_equal(lut[flip][:, :3], np.tile([2.0, 1.0, 0.0], (flip.sum(), 1)))
    assert np.array_equal(lut[flip][:, 3], 2 - 2 * af[flip]) and np.array_equal(lut[~flip][:, 3], 2 * af[~flip])
    ref = R.firth_ref(sm, src.packed[rows], lut)
    assert np.array_equal(got["beta.firth"][flagged], np.where(flip, -ref[:, 0], ref[:, 0]))     # negated where flipped
    assert np.array_equal(got["SE.firth"][flagged], ref[:, 1])
    assert np.all(np.isfinite(ref[:, :2]))
    # a flipped row is the same fit as its complement read the other way: the alt-allele effect of the golden row
    j = int(np.flatnonzero(flip)[0])
    codes = np.array([2, 1, 0, 3], dtype=np.uint8)
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    orig = pack_dosage_2bit(codes[unpack_dosage_2bit(src.packed[rows[j]:rows[j] + 1], sm.n)])
    lut_o, flip_o = firth.firth_tables(1 - af[j:j + 1])
    assert not flip_o[0]
    ref_o = R.firth_ref(sm, orig, lut_o)
    assert abs(got["beta.firth"][flagged][j] + ref_o[0, 0]) <= 1e-12 * abs(ref_o[0, 0])

    from saigegds_amd.assoc import seqAssocGLMM_SPA
    seqAssocGLMM_SPA(_source(60), mod, mac=4, verbose=True, firth_pval=0.05)
    assert "p-value threshold for Firth effect sizes: 0.05" in capsys.readouterr().out


def test_loco_runs_use_their_own_model(on_cpu):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    mod = load_null_model("saige_model.npz")
    src = _source(300)
    src.chromosome = ["1"] * 150 + ["2"] * 150
    rng = np.random.default_rng(3)
    mu = mod.fitted_values
    loco = {ch: {"fitted_values": np.clip(mu * rng.uniform(0.8, 1.2, mu.size), 1e-3, 1 - 1e-3)} for ch in ("1", "2")}
    got = seqAssocGLMM_SPA(src, replace(mod, loco=loco), mac=4, verbose=False, firth_pval=0.2)
    assert len(on_cpu) == 2
    for (mu_used, n_rows), ch in zip(on_cpu, ("1", "2")):
        assert np.array_equal(mu_used, loco[ch]["fitted_values"]) and n_rows > 0
    assert sum(n for _, n in on_cpu) == int((got["pval"] <= 0.2).sum()) == int(got["cvg.firth"].sum())


def test_rds_carries_the_columns(on_cpu, tmp_path):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    from saigegds_amd.results import seqSAIGE_LoadPval
    mod = load_null_model("saige_model.npz")
    want = seqAssocGLMM_SPA(_source(200), mod, mac=4, verbose=False, firth_pval=0.1)
    for name in ("r.rds", "r.RData"):
        fn = str(tmp_path / name)
        assert seqAssocGLMM_SPA(_source(200), mod, mac=4, verbose=False, firth_pval=0.1, res_savefn=fn) is None
        back = seqSAIGE_LoadPval(fn)
        for k in ("beta.firth", "SE.firth", "cvg.firth", "pval"):
            assert np.array_equal(np.asarray(back[k]), np.asarray(want[k]), equal_nan=k != "cvg.firth"), (name, k)


def test_refusals(on_cpu, tmp_path):
    from saigegds_amd.assoc import GenotypeSource, seqAssocGLMM_SPA
    from saigegds_amd.gds import unpack_dosage_2bit
    mod, src = load_null_model("saige_model.npz"), _source(40)
    with pytest.raises(ValueError, match="binary"):
        seqAssocGLMM_SPA(src, load_null_model("saige_model_quant.npz"), mac=4, verbose=False, firth_pval=0.05)
    ds = unpack_dosage_2bit(src.packed, len(src.sample_id())).astype(np.float64)
    ds[ds == 3] = np.nan
    ds[0, 0] = 0.5
    with pytest.raises(NotImplementedError, match="dosage input"):
        seqAssocGLMM_SPA(GenotypeSource(src.sample_id(), dosage=ds), mod, mac=4, verbose=False, firth_pval=0.05)
    with pytest.raises(NotImplementedError, match="dosage input"):      # an integer matrix with a value that is no hard call
        bad = np.where(np.isnan(ds), 255, ds).astype(np.uint8)
        bad[0, 0] = 7
        seqAssocGLMM_SPA(GenotypeSource(src.sample_id(), dosage=bad), mod, mac=4, verbose=False, firth_pval=0.05)
    with pytest.raises(ValueError, match="gds output has no columns"):
        seqAssocGLMM_SPA(src, mod, mac=4, verbose=False, firth_pval=0.05, res_savefn=str(tmp_path / "r.gds"))
    for bad in (0, 1.5, -0.1, "x", True):
        with pytest.raises(ValueError, match="firth_pval"):
            seqAssocGLMM_SPA(src, mod, mac=4, verbose=False, firth_pval=bad)
    with pytest.raises(ValueError, match="firth_maxit"):
        seqAssocGLMM_SPA(src, mod, mac=4, verbose=False, firth_pval=0.05, firth_maxit=0)
    assert on_cpu == []
    assert not os.path.exists(tmp_path / "r.gds")


def test_firth_pass_batches_and_skips_invalid_rows(monkeypatch):
    """firth_pass alone: batches of bounded bytes give what one batch gives; rows that are not valid are left out."""
    from saigegds_amd import firth
    from saigegds_amd.assoc import open_scan_input
    from saigegds_amd.nullmod import init_nullmod
    mod, src = load_null_model("saige_model.npz"), _source(120)
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    inp = open_scan_input(src, mod, "", False)
    sc = R.RefScanner(sm)
    out, valid = sc.scan_2bit(src.packed)
    sc.close()
    rows = np.arange(0, 120, 5)
    monkeypatch.setattr(R.RefScanner, "calls", [])
    one = firth.firth_pass(inp, out, valid, rows, lambda: R.RefScanner(sm), 50)
    assert len(R.RefScanner.calls) == 1
    monkeypatch.setattr(firth, "FIRTH_BATCH_BYTES", 7 * 250)
    many = firth.firth_pass(inp, out, valid, rows[::-1], lambda: R.RefScanner(sm), 50)
    assert len(R.RefScanner.calls) == 1 + -(-int((valid[rows] != 0).sum()) // 7)
    for a, b in zip(one, many):
        assert np.array_equal(a, b, equal_nan=True)
    keep = rows[valid[rows] != 0]
    off = np.setdiff1d(np.arange(120), keep)
    assert np.isnan(one[0][off]).all() and not one[2][off].any() and one[2][keep].all()
