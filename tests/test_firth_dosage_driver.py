"""seqAssocGLMM_SPA(firth_pval=) and firth_pass on dosage input, on the CPU: the golden genotypes with fractional values
as an in-memory float64 source through the stand-in scanner of tests/firth_ds_ref.py (the scan oracle and the long-double
Firth reference behind a dosage block with load / scan / firth).  No GPU."""
import os
from dataclasses import replace

import numpy as np
import pytest

import firth_ds_ref as D
import firth_ref as R
from conftest import GOLDEN, load_null_model
from skat_ds_ref import flip_mean

M = 600           # variants of the golden set the driver runs see
TODAY = ["id", "chr", "pos", "ref", "alt", "AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged"]


def _dosages(m=M):
    """The first m golden variants as float64 dosages: every 7th row alt-major, missing = NaN, and every non-zero
    dosage scaled by a factor in [0.75, 1] (a multiple of 1 / 64: the rows' sums are exact in double)."""
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    sid = [str(s) for s in g["sample_id"]]
    codes = unpack_dosage_2bit(g["packed"][:m], len(sid))
    codes[::7] = np.array([2, 1, 0, 3], dtype=np.uint8)[codes[::7]]
    rng = np.random.default_rng(21)
    ds = codes.astype(np.float64) * (1 - rng.integers(0, 17, codes.shape) / 64.0)
    ds[codes == 3] = np.nan
    return g, sid, ds


def _source(m=M):
    from saigegds_amd.assoc import GenotypeSource
    g, sid, ds = _dosages(m)
    return GenotypeSource(sid, dosage=ds, variant_id=g["variant_id"][:m], position=g["position"][:m])


class CountingScanner(D.RefDsScanner):
    scans = []           # rows of every scan call

    def scan_f64(self, dosage):
        CountingScanner.scans.append(np.asarray(dosage).shape[0])
        return super().scan_f64(dosage)


@pytest.fixture()
def on_cpu(monkeypatch):
    """The driver with the stand-in for the device: one visible device, CountingScanner for Scanner."""
    from saigegds_amd import _lib
    real = _lib.load()

    class OneDevice:
        def __getattr__(self, name):
            return getattr(real, name)

        def sgx_device_count(self):
            return 1

    monkeypatch.setattr(_lib, "load", OneDevice)
    monkeypatch.setattr(_lib, "Scanner", CountingScanner)
    monkeypatch.setattr(D.RefDsScanner, "calls", [])
    monkeypatch.setattr(CountingScanner, "scans", [])
    return D.RefDsScanner.calls


@pytest.fixture(scope="module")
def runs():
    return {}


def _run(runs, key, **kw):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    if key not in runs:
        runs[key] = seqAssocGLMM_SPA(_source(), load_null_model("saige_model.npz"), mac=4, verbose=False, **kw)
    return runs[key]


def test_columns_on_the_flagged_rows(on_cpu, runs):
    from saigegds_amd.nullmod import init_nullmod
    plain = _run(runs, "plain")
    assert on_cpu == [] and list(plain) == TODAY                # without firth_pval: no call and no column
    got = _run(runs, "firth", firth_pval=0.05)
    assert list(got) == TODAY + ["beta.firth", "SE.firth", "cvg.firth"]
    for k in TODAY:                                             # the scan's own columns are unchanged
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    flagged = got["pval"] <= 0.05
    assert 10 < flagged.sum() < flagged.size
    assert np.isnan(got["beta.firth"][~flagged]).all() and np.isnan(got["SE.firth"][~flagged]).all()
    assert got["cvg.firth"].dtype == bool and not got["cvg.firth"][~flagged].any() and got["cvg.firth"][flagged].all()
    assert len(on_cpu) == 1 and on_cpu[0][1] == int(flagged.sum())

    # the reference on those rows, straight from the dosage rows and their own counts
    mod = load_null_model("saige_model.npz")
    g, _, ds = _dosages()
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    rows = ds[np.isin(g["variant_id"][:M], got["id"][flagged])]
    flip, mean = flip_mean(rows)
    assert flip.any() and not flip.all()                        # alt-major rows are among the flagged ones
    assert np.array_equal(flip != 0, got["AF.alt"][flagged] > 0.5)
    assert any((r[np.isfinite(r)] % 1 != 0).any() for r in rows)                      # fractional values
    ref = D.firth_ds_ref(sm, rows, flip, mean)
    assert np.all(np.isfinite(ref[:, :2]))
    assert np.array_equal(got["beta.firth"][flagged], np.where(flip != 0, -ref[:, 0], ref[:, 0]))      # negated where flipped
    assert np.array_equal(got["SE.firth"][flagged], ref[:, 1])


def test_firth_pass_batches_equal_one_batch(monkeypatch):
    from saigegds_amd import aggregate, firth
    from saigegds_amd.assoc import open_scan_input
    from saigegds_amd.nullmod import init_nullmod
    mod, src = load_null_model("saige_model.npz"), _source(120)
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    inp = firth.firth_input(open_scan_input(src, mod, "", False, any_matrix=True), D.RefDsScanner)
    assert inp.kind == "dosage" and inp.ds_dtype == np.float64
    sc = D.RefDsScanner(sm)
    out, valid = sc.scan_f64(src.dosage)
    sc.close()
    rows = np.arange(0, 120, 5)
    monkeypatch.setattr(D.RefDsScanner, "calls", [])
    one = firth.firth_pass(inp, out, valid, rows, lambda: D.RefDsScanner(sm), 50)
    assert len(D.RefDsScanner.calls) == 1
    monkeypatch.setattr(aggregate, "DS_BUDGET", 7 * aggregate.ds_row_bytes(np.float64, sm.n))
    many = firth.firth_pass(inp, out, valid, rows[::-1], lambda: D.RefDsScanner(sm), 50)
    n_ok = int((valid[rows] != 0).sum())
    assert len(D.RefDsScanner.calls) == 1 + -(-n_ok // 7)
    assert [n for _, n in D.RefDsScanner.calls[1:]] == [7] * (n_ok // 7) + ([n_ok % 7] if n_ok % 7 else [])
    for a, b in zip(one, many):
        assert np.array_equal(a, b, equal_nan=True)
    keep = rows[valid[rows] != 0]
    off = np.setdiff1d(np.arange(120), keep)
    assert np.isnan(one[0][off]).all() and not one[2][off].any() and one[2][keep].all()


def test_loco_runs_use_their_own_model(on_cpu):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    mod = load_null_model("saige_model.npz")
    src = _source(300)
    src.chromosome = ["1"] * 150 + ["2"] * 150
    rng = np.random.default_rng(3)
    mu = mod.fitted_values
    loco = {ch: {"fitted_values": np.clip(mu * rng.uniform(0.8, 1.2, mu.size), 1e-3, 1 - 1e-3)} for ch in ("1", "2")}
    got = seqAssocGLMM_SPA(src, replace(mod, loco=loco), mac=4, verbose=False, firth_pval=0.2)
    assert len(on_cpu) == 2                                    # one block, of a scanner of its own model, per chromosome
    for (mu_used, n_rows), ch in zip(on_cpu, ("1", "2")):
        assert np.array_equal(mu_used, loco[ch]["fitted_values"]) and n_rows > 0
    assert sum(n for _, n in on_cpu) == int((got["pval"] <= 0.2).sum()) == int(got["cvg.firth"].sum())


def test_rds_carries_the_columns(on_cpu, tmp_path):
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    from saigegds_amd.results import seqSAIGE_LoadPval
    mod = load_null_model("saige_model.npz")
    want = seqAssocGLMM_SPA(_source(200), mod, mac=4, verbose=False, firth_pval=0.1)
    assert want["cvg.firth"].any()
    fn = str(tmp_path / "r.rds")
    assert seqAssocGLMM_SPA(_source(200), mod, mac=4, verbose=False, firth_pval=0.1, res_savefn=fn) is None
    back = seqSAIGE_LoadPval(fn)
    for k in ("beta.firth", "SE.firth", "cvg.firth", "pval"):
        assert np.array_equal(np.asarray(back[k]), np.asarray(want[k]), equal_nan=k != "cvg.firth"), k


def test_a_scanner_that_cannot_serve_dosages_is_refused_unscanned(on_cpu, monkeypatch):
    from saigegds_amd import _lib, firth
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    mod, src = load_null_model("saige_model.npz"), _source(40)

    class NoBlock(R.RefScanner):                                # a scanner class without dosage_block
        def scan_f64(self, dosage):
            CountingScanner.scans.append(np.asarray(dosage).shape[0])
            return self._o.scan_f64(dosage)

    class NoFirthBlock:
        load, scan, close, __enter__, __exit__, __init__ = (getattr(D._RefDsBlock, k) for k in
                                                            ("load", "scan", "close", "__enter__", "__exit__", "__init__"))

    class NoFirth(CountingScanner):                             # a block without firth
        block_type = NoFirthBlock

    for cls in (NoBlock, NoFirth):
        monkeypatch.setattr(_lib, "Scanner", cls)
        with pytest.raises(NotImplementedError, match="dosage input") as e:
            seqAssocGLMM_SPA(src, mod, mac=4, verbose=False, firth_pval=0.05)
        assert str(e.value) == firth.NO_DOSAGE
        assert CountingScanner.scans == [] and on_cpu == [], cls.__name__
        got = seqAssocGLMM_SPA(src, mod, mac=4, verbose=False)                      # without firth_pval it scans
        assert len(got["pval"]) > 0 and CountingScanner.scans != []
        monkeypatch.setattr(CountingScanner, "scans", [])
