"""CPU: the host logic of seqFitDenseGRM / seqFitSparseGRM (saigegds_amd/grm.py) with the numpy stand-in operator of
grm_dense_ref.py injected, on the reference's golden file; and seqSAIGE_LoadPval over the three result writers."""
import os

import numpy as np
import pytest

import grm_dense_ref as D
from saigegds_amd import SparseGRM, seqFitDenseGRM, seqFitSparseGRM, seqSAIGE_LoadPval
from saigegds_amd.rds import read_rds

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GDS = os.path.join(GOLD, "grm1k_10k_snp.gds")
ARGS = dict(maf=0.005, missing_rate=0.01, max_num_snp=2000, seed=200)


class _Spy(D.NumpyGrm):
    last = None

    def __init__(self, packed, n):
        super().__init__(packed, n)
        _Spy.last = self


def _fit_markers():
    """The packed markers seqFitNullGLMM_SPA hands its operator with the same arguments."""
    from saigegds_amd.fitnull import seqFitNullGLMM_SPA
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    data = {"sample.id": ph["sample_id"], "y": ph["y"], "x1": ph["x1"], "x2": ph["x2"]}
    got = {}

    class Stop(Exception):
        pass

    def factory(packed, n):
        got["packed"], got["n"] = packed, n
        raise Stop()

    with pytest.raises(Stop):
        seqFitNullGLMM_SPA("y ~ x1 + x2", data, GDS, verbose=False, operator_factory=factory, **ARGS)
    return got


def test_markers_are_those_of_the_null_model_fit():
    want = _fit_markers()
    ids, K = seqFitDenseGRM(GDS, verbose=False, operator_factory=_Spy, **ARGS)
    assert _Spy.last.n == want["n"] == 1000 == len(ids) and K.shape == (1000, 1000)
    assert _Spy.last.packed.shape[0] == 2000 and np.array_equal(_Spy.last.packed, want["packed"])
    assert np.array_equal(K, _Spy.last.K)
    sp = seqFitSparseGRM(GDS, verbose=False, operator_factory=_Spy, **ARGS)
    assert np.array_equal(_Spy.last.packed, want["packed"])
    assert isinstance(sp, SparseGRM) and sp.n == 1000 and sp.n_markers == 2000 and sp.rel_cutoff == 0.125
    assert sp.sample_id == ids
    wi, wj, wx = D.threshold(K, 0.125)
    assert np.array_equal(sp.i, wi) and np.array_equal(sp.j, wj) and np.array_equal(sp.x, wx)
    b = np.random.default_rng(3).standard_normal(sp.n)
    np.testing.assert_allclose(sp.matvec(b), sp.to_dense() @ b, rtol=0, atol=1e-12 * np.abs(sp.to_dense()).sum(axis=1).max())
    pairs = sp.related_pairs()
    assert len(pairs) == int((sp.i != sp.j).sum()) and all(a != c and v >= 0.125 for a, c, v in pairs)


def test_sample_subset_and_order_are_respected():
    ids_all, _ = seqFitDenseGRM(GDS, verbose=False, operator_factory=D.NumpyGrm, variant_id=range(1, 501))
    pick = [ids_all[k] for k in (700, 3, 512, 44, 45, 999, 0)]
    ids, K = seqFitDenseGRM(GDS, sample_id=pick, verbose=False, operator_factory=_Spy, variant_id=range(1, 501))
    assert ids == pick and _Spy.last.n == len(pick)
    ids_g, K_g = seqFitDenseGRM(GDS, sample_id=(s for s in pick), verbose=False, operator_factory=D.NumpyGrm,
                                variant_id=range(1, 501))
    assert ids_g == pick and np.array_equal(K_g, K)           # any iterable, a generator included
    srt = sorted(range(len(pick)), key=lambda k: ids_all.index(pick[k]))
    ids_s, K_s = seqFitDenseGRM(GDS, sample_id=[pick[k] for k in srt], verbose=False, operator_factory=D.NumpyGrm,
                                variant_id=range(1, 501))
    assert np.array_equal(K[np.ix_(srt, srt)], K_s)            # the same numbers, in the caller's order
    sp = seqFitSparseGRM(GDS, sample_id=pick, rel_cutoff=-0.05, verbose=False, operator_factory=D.NumpyGrm,
                         variant_id=range(1, 501))
    assert sp.sample_id == pick and np.all(sp.i <= sp.j)
    assert np.array_equal(np.lexsort((sp.j, sp.i)), np.arange(sp.i.size))
    wi, wj, wx = D.threshold(K, -0.05)
    assert np.array_equal(sp.i, wi) and np.array_equal(sp.j, wj) and np.array_equal(sp.x, wx)
    with pytest.raises(ValueError, match="not in the GDS file"):
        seqFitDenseGRM(GDS, sample_id=["nobody"], verbose=False, operator_factory=D.NumpyGrm)
    with pytest.raises(ValueError, match="unique"):
        seqFitSparseGRM(GDS, sample_id=[pick[0], pick[0]], verbose=False, operator_factory=D.NumpyGrm)


def test_files_round_trip(tmp_path):
    kw = dict(verbose=False, operator_factory=D.NumpyGrm, variant_id=range(1, 301))
    pick = [str(s) for s in np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))["sample_id"][:40]]
    for ext in ("rds", "npz"):
        fn = str(tmp_path / ("sp." + ext))
        sp = seqFitSparseGRM(GDS, sample_id=pick, rel_cutoff=0.05, out_fn=fn, **kw)
        fd = str(tmp_path / ("de." + ext))
        ids, K = seqFitDenseGRM(GDS, sample_id=pick, out_fn=fd, **kw)
        if ext == "rds":
            r = read_rds(fn)
            assert r.names == ["sample.id", "i", "j", "x", "n", "rel.cutoff"]
            got = {k: r[k] for k in r.names}
            d = read_rds(fd)
            assert d.names == ["sample.id", "grm"] and list(d["sample.id"]) == ids
            assert np.array_equal(np.asarray(d["grm"]), K)
        else:
            z = np.load(fn)
            got = {"sample.id": z["sample_id"], "i": z["i"], "j": z["j"], "x": z["x"], "n": [z["n"]],
                   "rel.cutoff": [z["rel_cutoff"]]}
            d = np.load(fd)
            assert list(d["sample_id"]) == ids and np.array_equal(d["K"], K)
        assert [str(s) for s in got["sample.id"]] == sp.sample_id
        assert np.array_equal(np.asarray(got["i"]), sp.i + 1) and np.array_equal(np.asarray(got["j"]), sp.j + 1)
        assert np.array_equal(np.asarray(got["x"]), sp.x)
        assert int(np.asarray(got["n"])[0]) == 40 and float(np.asarray(got["rel.cutoff"])[0]) == 0.05
    with pytest.raises(ValueError, match="Unknown format"):
        seqFitSparseGRM(GDS, out_fn=str(tmp_path / "x.txt"), **kw)


def test_dense_refuses_what_does_not_fit(monkeypatch):
    import saigegds_amd.grm as G
    monkeypatch.setattr(G, "DENSE_BUDGET_BYTES", 8 * 999 * 999)
    with pytest.raises(ValueError, match="seqFitSparseGRM"):
        seqFitDenseGRM(GDS, verbose=False, operator_factory=D.NumpyGrm)
    assert G.SparseGRM is SparseGRM and 8 * 32768 ** 2 <= 8 << 30
    with pytest.raises(ValueError, match="finite"):
        seqFitSparseGRM(GDS, rel_cutoff=float("nan"), verbose=False, operator_factory=D.NumpyGrm)


def test_load_pval_round_trips_the_three_writers(tmp_path):
    from saigegds_amd.results import save_result
    z = np.load(os.path.join(GOLD, "saige_pval.npz"))
    ans = {"id": z["id"].astype(np.int32), "chr": [str(s) for s in z["chr"]], "AF.alt": z["AF_alt"],
           "num": z["num"].astype(np.int32), "beta": z["beta"], "pval": z["pval"], "converged": z["converged"]}
    m = len(ans["chr"])
    for ext in ("rds", "RData", "gds"):
        fn = str(tmp_path / ("res." + ext))
        save_result(ans, fn, "LZMA", sample_id=["s1", "s2"])
        r = seqSAIGE_LoadPval(fn)
        assert list(r) == list(ans), ext
        for k, v in ans.items():
            if isinstance(v, list):
                assert list(r[k]) == v, (ext, k)
            else:
                assert np.array_equal(np.asarray(r[k]), v, equal_nan=v.dtype.kind == "f"), (ext, k)
        assert np.asarray(r["converged"]).dtype == bool
        sub = seqSAIGE_LoadPval(fn, varnm=["pval", "chr"], index=np.array([5, 2, m - 1]))
        assert list(sub) == ["pval", "chr"]
        assert np.array_equal(sub["pval"], ans["pval"][[5, 2, m - 1]], equal_nan=True)
        assert list(sub["chr"]) == [ans["chr"][k] for k in (5, 2, m - 1)]
        mask = np.zeros(m, dtype=bool)
        mask[10:13] = True
        assert np.array_equal(seqSAIGE_LoadPval(fn, ["id"], mask)["id"], ans["id"][10:13])
        with pytest.raises(KeyError):
            seqSAIGE_LoadPval(fn, varnm=["nope"])
    both = seqSAIGE_LoadPval([str(tmp_path / "res.rds"), str(tmp_path / "res.gds")], varnm=["id", "chr"])
    assert np.array_equal(both["id"], np.concatenate([ans["id"], ans["id"]])) and both["chr"] == ans["chr"] * 2
    with pytest.raises(ValueError, match="index"):
        seqSAIGE_LoadPval([str(tmp_path / "res.rds")] * 2, index=[0])
    with pytest.raises(ValueError, match="Unknown format"):
        seqSAIGE_LoadPval(str(tmp_path / "res.txt"))
