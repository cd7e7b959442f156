"""seqAssocGLMM_SPA(exact_mac=) and exact_pass on the CPU: golden genotypes thinned to a few carriers and the golden model
through the stand-in scanner of tests/exact_ref.py (the scan oracle and the rational reference).  No GPU."""
import os
from dataclasses import replace

import numpy as np
import pytest

import exact_ref as R
from conftest import GOLDEN, load_null_model

M = 240           # variants the driver runs see
TODAY = ["id", "chr", "pos", "ref", "alt", "AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged"]
EXACT = ["pval.exact", "pval.exact.full"]


def _codes(m=M):
    """The first m golden variants; two rows of three keep only their first 1 + (row mod 14) carriers, every 5th row
    has two missing genotypes, every 7th is turned alt-major (codes 0 and 2 swapped)."""
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:m], len(g["sample_id"]))
    for j in range(m):
        if j % 3:
            car = np.flatnonzero(codes[j])
            codes[j, car[1 + j % 14:]] = 0
        if j % 5 == 0:
            codes[j, [17 + j, 500 + j]] = 3
    codes[::7] = np.array([2, 1, 0, 3], dtype=np.uint8)[codes[::7]]
    return g, codes


def _source(m=M, as_matrix=None):
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit
    g, codes = _codes(m)
    sid = [str(s) for s in g["sample_id"]]
    if as_matrix is not None:
        ds = codes.astype(as_matrix)
        ds[codes == 3] = 255
        return GenotypeSource(sid, dosage=ds, variant_id=g["variant_id"][:m], position=g["position"][:m])
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
    monkeypatch.setattr(R.RefScanner, "exact_calls", [])
    monkeypatch.setattr(R.RefScanner, "calls", [])
    return R.RefScanner.exact_calls


@pytest.fixture(scope="module")
def runs():
    return {}


def _run(runs, key, **kw):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    if key not in runs:
        runs[key] = seqAssocGLMM_SPA(_source(), load_null_model("saige_model.npz"), mac=kw.pop("mac", 1), verbose=False, **kw)
    return runs[key]


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


def test_none_changes_nothing(on_cpu, runs):
    plain, none = _run(runs, "plain"), _run(runs, "none", exact_mac=None)
    assert list(plain) == list(none) == TODAY
    _same(plain, none, TODAY)
    assert on_cpu == []                                        # no exact call was made


def test_columns_on_the_rare_rows(on_cpu, runs, capsys):
    from saigegds_amd import firth
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    plain, got = _run(runs, "plain"), _run(runs, "exact", exact_mac=10)
    assert list(got) == TODAY + EXACT
    _same(plain, got, TODAY)
    rare = got["mac"] <= 10
    assert 50 < rare.sum() < rare.size
    assert np.isnan(got["pval.exact"][~rare]).all() and np.isnan(got["pval.exact.full"][~rare]).all()
    assert np.isfinite(got["pval.exact"][rare]).all()
    assert np.all((got["pval.exact"][rare] > 0) & (got["pval.exact"][rare] <= got["pval.exact.full"][rare]))
    assert len(on_cpu) == 1 and on_cpu[0][1:] == (int(rare.sum()), 10)

    # the reference on those rows, straight from the codes and the AF column
    mod = load_null_model("saige_model.npz")
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 1, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    g, codes = _codes()
    rows = np.flatnonzero(np.isin(g["variant_id"][:M], got["id"][rare]))
    lut, flip = firth.firth_tables(got["AF.alt"][rare])
    assert flip.any() and not flip.all()                       # alt-major rows are among the rare ones
    assert (codes[rows] == 3).any()
    ref = R.exact_ref(sm.mu, sm.y, pack_dosage_2bit(codes[rows]), lut, 10)
    assert np.all(ref[:, 3] == 1) and np.array_equal(ref[:, 2], got["mac"][rare])
    assert np.array_equal(got["pval.exact"][rare], ref[:, 0]) and np.array_equal(got["pval.exact.full"][rare], ref[:, 1])

    # rows the scan's own mac filter dropped are not in the table at all, whatever exact_mac says
    at4 = _run(runs, "mac4", mac=4, exact_mac=10)
    assert at4["mac"].min() >= 4 and len(at4["id"]) < len(got["id"])
    keep = np.isin(got["id"], at4["id"])
    _same({k: np.asarray(got[k])[keep] for k in TODAY + EXACT}, at4, TODAY + EXACT)

    from saigegds_amd.assoc import seqAssocGLMM_SPA
    seqAssocGLMM_SPA(_source(30), mod, mac=2, verbose=True, exact_mac=7)
    text = capsys.readouterr().out
    assert "MAC threshold for exact p-values: 7" in text and "lower `mac`" in text


def test_loco_runs_use_their_own_model(on_cpu):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    mod = load_null_model("saige_model.npz")
    src = _source(120)
    src.chromosome = ["1"] * 60 + ["2"] * 60
    rng = np.random.default_rng(3)
    mu = mod.fitted_values
    loco = {ch: {"fitted_values": np.clip(mu * rng.uniform(0.8, 1.2, mu.size), 1e-3, 1 - 1e-3)} for ch in ("1", "2")}
    got = seqAssocGLMM_SPA(src, replace(mod, loco=loco), mac=1, verbose=False, exact_mac=10)
    assert len(on_cpu) == 2
    for (mu_used, n_rows, mm), ch in zip(on_cpu, ("1", "2")):
        assert np.array_equal(mu_used, loco[ch]["fitted_values"]) and n_rows > 0 and mm == 10
    assert sum(c[1] for c in on_cpu) == int((got["mac"] <= 10).sum()) == int(np.isfinite(got["pval.exact"]).sum())
    full = seqAssocGLMM_SPA(src, mod, mac=1, verbose=False, exact_mac=10)     # and the models matter
    assert not np.array_equal(full["pval.exact"], got["pval.exact"], equal_nan=True)


def test_together_with_firth(on_cpu, runs):
    both = _run(runs, "both", exact_mac=10, firth_pval=0.05)
    firth, exact = _run(runs, "firth", firth_pval=0.05), _run(runs, "exact", exact_mac=10)
    assert list(both) == TODAY + ["beta.firth", "SE.firth", "cvg.firth"] + EXACT
    _same(both, firth, TODAY + ["beta.firth", "SE.firth", "cvg.firth"])
    _same(both, exact, EXACT)
    assert both["cvg.firth"].any()


def test_rds_carries_the_columns(on_cpu, tmp_path):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    from saigegds_amd.results import seqSAIGE_LoadPval
    mod = load_null_model("saige_model.npz")
    want = seqAssocGLMM_SPA(_source(60), mod, mac=1, verbose=False, exact_mac=10)
    for name in ("r.rds", "r.RData"):
        fn = str(tmp_path / name)
        assert seqAssocGLMM_SPA(_source(60), mod, mac=1, verbose=False, exact_mac=10, res_savefn=fn) is None
        back = seqSAIGE_LoadPval(fn)
        _same(back, want, EXACT + ["pval"])


def test_a_hard_call_matrix_gives_the_packed_columns(on_cpu, runs):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    mod = load_null_model("saige_model.npz")
    want = seqAssocGLMM_SPA(_source(60), mod, mac=1, verbose=False, exact_mac=10)
    got = seqAssocGLMM_SPA(_source(60, as_matrix=np.uint8), mod, mac=1, verbose=False, exact_mac=10)
    assert np.isfinite(got["pval.exact"]).any()
    _same(got, want, EXACT + ["mac", "AF.alt"])


def test_refusals(on_cpu, tmp_path):
    from saigegds_amd.assoc import GenotypeSource, seqAssocGLMM_SPA
    from saigegds_amd.gds import unpack_dosage_2bit
    mod, src = load_null_model("saige_model.npz"), _source(40)
    with pytest.raises(ValueError, match="binary"):
        seqAssocGLMM_SPA(src, load_null_model("saige_model_quant.npz"), mac=1, verbose=False, exact_mac=10)
    ds = unpack_dosage_2bit(src.packed, len(src.sample_id())).astype(np.float64)
    ds[ds == 3] = np.nan
    ds[0, 0] = 0.5
    with pytest.raises(NotImplementedError, match="hard calls"):
        seqAssocGLMM_SPA(GenotypeSource(src.sample_id(), dosage=ds), mod, mac=1, verbose=False, exact_mac=10)
    with pytest.raises(NotImplementedError, match="hard calls"):       # an integer matrix with a value that is no hard call
        bad = np.where(np.isnan(ds), 255, ds).astype(np.uint8)
        bad[0, 0] = 7
        seqAssocGLMM_SPA(GenotypeSource(src.sample_id(), dosage=bad), mod, mac=1, verbose=False, exact_mac=10)
    with pytest.raises(ValueError, match="gds output has no columns"):
        seqAssocGLMM_SPA(src, mod, mac=1, verbose=False, exact_mac=10, res_savefn=str(tmp_path / "r.gds"))
    for bad in (0, 64, 2.5, True, -3, "4"):
        with pytest.raises(ValueError, match="exact_mac"):
            seqAssocGLMM_SPA(src, mod, mac=1, verbose=False, exact_mac=bad)
    assert on_cpu == [] and R.RefScanner.calls == []             # ... all of them before any row was scanned
    assert not os.path.exists(tmp_path / "r.gds")


def test_exact_pass_batches_and_skips_invalid_rows(on_cpu, monkeypatch):
    """exact_pass alone: batches of bounded bytes give what one batch gives; rows that are not valid, and rows with
    more minor alleles than max_mac, are left NaN."""
    from saigegds_amd import exact, firth
    from saigegds_amd.assoc import open_scan_input
    from saigegds_amd.nullmod import init_nullmod
    mod, src = load_null_model("saige_model.npz"), _source(120)
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 3, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    inp = open_scan_input(src, mod, "", False)
    sc = R.RefScanner(sm)
    out, valid = sc.scan_2bit(src.packed)
    sc.close()
    rows = np.arange(0, 120, 2)
    one = exact.exact_pass(inp, out, valid, rows, lambda: R.RefScanner(sm), 8)
    assert len(on_cpu) == 1
    monkeypatch.setattr(firth, "FIRTH_BATCH_BYTES", 7 * 250)
    many = exact.exact_pass(inp, out, valid, rows[::-1], lambda: R.RefScanner(sm), 8)
    assert len(on_cpu) == 1 + -(-int((valid[rows] != 0).sum()) // 7)
    for a, b in zip(one, many):
        assert np.array_equal(a, b, equal_nan=True)
    ok = rows[(valid[rows] != 0) & (out[rows, 1] <= 8)]
    off = np.setdiff1d(np.arange(120), ok)
    assert ok.size > 10 and (valid[rows] == 0).any() and (out[rows, 1] > 8).any()
    assert np.isnan(one[0][off]).all() and np.isnan(one[1][off]).all() and np.isfinite(one[0][ok]).all()
