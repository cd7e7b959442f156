"""The null-model fit on a file that holds only imputed dosages (annotation/format/DS, no genotype node): the package's
numpy statement of the rounding rule, the marker loader on written files, and -- with the CPU oracle's GRM operator
injected -- a fit and a GxG call.  No GPU."""
import os

import numpy as np
import pytest

import ds_quant_cases as Q
import packed_ds_cases as P
from saigegds_amd.assoc import GenotypeSource
from saigegds_amd.fitnull import _load_grm_markers, seqFitNullGLMM_SPA
from saigegds_amd.gds import GdsFile, pack_dosage_2bit, quantize_dosage_2bit, round_dosage_codes, unpack_dosage_2bit

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ARRAYS = ("tau", "coefficients", "fitted_values", "linear_predictors", "residuals", "cov", "y", "V", "X1", "XV",
          "XXVX_inv", "mu_noK", "res_noK", "var_ratio", "variant_id")


def _markers(gdsfile, sample_id, maf=0.005, missing_rate=0.01, variant_id=None, max_num_snp=1000000):
    """``_load_grm_markers`` for a model y ~ x on the given samples, the way a fit with an injected operator calls it."""
    n = len(sample_id)
    cols = {"y": np.arange(n, dtype=np.float64) % 2, "x": np.linspace(0, 1, n)}
    return _load_grm_markers("y", ["x"], cols, [str(s) for s in sample_id], gdsfile, maf, missing_rate, max_num_snp,
                             variant_id, 200, False, use_gpu_counts=False)


def _same_markers(a, b):
    assert a["n_samp"] == b["n_samp"] and list(a["sample_id"]) == list(b["sample_id"])
    assert np.array_equal(a["idx"], b["idx"])
    assert a["packed"].dtype == np.uint8 and np.array_equal(a["packed"], b["packed"])


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_rule_on_the_edge_rows(cls):
    """The package's statement gives the expected code at every boundary the class represents, and agrees with the
    test helper's statement on the whole output (ds_sum exactly: dyadic scales; float32, whose edge row holds +-1e30,
    within the bound of a reordered double sum, 4 n 2^-53 sum|v|)."""
    scale, offset = P.DYADIC[cls]
    for n in (3, 64, 257):
        raw, where = Q.edge_rows(cls, n)
        pk, nv, sm, dv, ds = quantize_dosage_2bit(raw, cls, scale, offset)
        codes = unpack_dosage_2bit(pk, n)
        assert len(where) == len(Q.edge_list(cls)) >= 9
        for r, c, code in where:
            assert codes[r, c] == code, (cls, n, r, c)
        r_pk, r_nv, r_sm, r_dv, r_ds, r_abs = Q.ref_quantize(raw, cls, scale, offset)
        assert np.array_equal(pk, r_pk) and np.array_equal(nv, r_nv) and np.array_equal(sm, r_sm)
        assert np.array_equal(dv, r_dv)
        assert np.all(np.abs(ds - r_ds) <= (4.0 * n * 2.0 ** -53 * r_abs if cls == "dFloat32" else 0.0))
    v = np.array([1e30, -1e30, -0.4, -0.0, np.nan, np.inf, 0.49999999999999994, 2.5, 2.4999999999999996])
    assert round_dosage_codes(v).tolist() == [3, 3, 0, 0, 3, 3, 0, 3, 2]


def test_rule_with_a_selection():
    raw, scale, offset, _ = Q.parity_rows("dPackedReal16", 65, seed=4)
    wide, sel = P.widen(raw, 102, seed=5)
    got = quantize_dosage_2bit(wide, "dPackedReal16", scale, offset, sel=sel, block_bytes=8 * 65 * 3)    # three rows a pass
    for a, b in zip(got, Q.ref_quantize(wide, "dPackedReal16", scale, offset, sel)):
        assert np.array_equal(a, b)


def test_hard_call_file_gives_the_source_s_markers(tmp_path):
    codes, sid = P.golden_codes(600)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    src = GenotypeSource(sid, packed=pack_dosage_2bit(codes))
    for cls in ("dPackedReal8U", "dPackedReal16", "dFloat32"):
        scale, offset = P.DYADIC[cls]
        fn = P.write_ds_file(tmp_path / f"{cls}.gds", P.encode(x, cls, scale, offset), cls, scale, offset, sid)
        got, ref = _markers(fn, sid), _markers(src, sid)
        assert 0 < ref["idx"].size < 600                  # the filter drops some and keeps some
        _same_markers(got, ref)
        assert np.array_equal(got["var_ids"], ref["var_ids"])
        # max_num_snp: the same draw from the same kept set
        _same_markers(_markers(fn, sid, max_num_snp=50), _markers(src, sid, max_num_snp=50))


def test_blurred_dosages_round_back_to_the_calls(tmp_path):
    codes, sid = P.golden_codes(300)
    rng = np.random.default_rng(11)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    blur = np.clip(x + rng.uniform(-0.3, 0.3, x.shape), 0, 2)
    ids = list(range(5, 300, 7))
    src = GenotypeSource(sid, packed=pack_dosage_2bit(codes))
    for cls in ("dPackedReal16U", "dFloat32"):
        scale, offset = P.DYADIC[cls]
        fn = P.write_ds_file(tmp_path / f"b_{cls}.gds", P.encode(blur, cls, scale, offset), cls, scale, offset, sid)
        got, ref = _markers(fn, sid, variant_id=ids), _markers(src, sid, variant_id=ids)
        assert ref["idx"].size == len(ids)
        _same_markers(got, ref)


def test_subset_of_the_samples_in_another_order(tmp_path):
    """40 samples in the file, `data` names 29 of them in another order: rows in the FILE's order."""
    rng = np.random.default_rng(12)
    sid = [f"s{i}" for i in range(40)]
    x = P.dosages(50, 40, 13)
    cls = "dPackedReal8"
    scale, offset = P.DYADIC[cls]
    raw = P.encode(x, cls, scale, offset)
    fn = P.write_ds_file(tmp_path / "sub.gds", raw, cls, scale, offset, sid)
    named = [sid[i] for i in rng.permutation(40)[:29]]
    in_file = sorted(sid.index(s) for s in named)
    ids = list(range(1, 51))
    got = _markers(fn, named, variant_id=ids)
    assert got["n_samp"] == 29 and got["sample_id"] == [sid[i] for i in in_file]
    want = Q.ref_quantize(raw, cls, scale, offset, sel=np.array(in_file))[0]
    assert np.array_equal(got["packed"], want) and np.array_equal(got["idx"], np.arange(50))
    # and through the filter: the counts are those of the selected columns
    flt = _markers(fn, named, maf=0.05, missing_rate=0.1)
    _, _, _, dv, ds, _ = Q.ref_quantize(raw, cls, scale, offset, sel=np.array(in_file))
    with np.errstate(invalid="ignore", divide="ignore"):
        af = ds / (2.0 * dv)
    keep = np.flatnonzero((np.minimum(af, 1 - af) >= 0.05) & ((29 - dv) / 29 <= 0.1))
    assert 0 < keep.size < 50
    assert np.array_equal(flt["idx"], keep) and np.array_equal(flt["packed"], want[keep])


def test_filter_takes_the_real_dosages(tmp_path):
    """N = 100, maf 0.05, missing rate 0.1, every constructed figure at least 1e-3 from its threshold.
    row 0: 20 samples at 0.4375 -> real maf 0.04375 (out), codes all 0 -> code maf 0 (out either way: control)
    row 1: 12 samples at 0.5625, the rest 0 -> real maf 0.03375 (OUT), codes 12 x 1 -> code maf 0.06 (in)
    row 2: 30 samples at 0.4375, the rest 0 -> real maf 0.065625 (IN), codes all 0 -> code maf 0 (out)
    row 3: 15 samples at 1 -> maf 0.075 both ways (in); row 4: the same with 12 missing (missing rate 0.12: out)
    row 5: row 3 with 8 missing: missing rate 0.08 (in), maf 15 / 184 = 0.0815."""
    n = 100
    x = np.zeros((6, n))
    x[0, :20] = 0.4375
    x[1, :12] = 0.5625
    x[2, :30] = 0.4375
    x[3, :15] = x[4, :15] = x[5, :15] = 1.0
    x[4, 50:62] = np.nan
    x[5, 50:58] = np.nan
    sid = [f"s{i}" for i in range(n)]
    for cls in ("dPackedReal8U", "dFloat32"):
        scale, offset = P.DYADIC[cls]
        fn = P.write_ds_file(tmp_path / f"f_{cls}.gds", P.encode(x, cls, scale, offset), cls, scale, offset, sid)
        got = _markers(fn, sid, maf=0.05, missing_rate=0.1)
        assert got["idx"].tolist() == [2, 3, 5], cls
        assert np.array_equal(got["packed"], pack_dosage_2bit(Q.ref_codes(x))[[2, 3, 5]])
        # the rounded codes would have kept another set
        codes = Q.ref_codes(x)
        ok = codes != 3
        af = np.where(ok, codes, 0).sum(axis=1) / (2.0 * ok.sum(axis=1))
        by_codes = np.flatnonzero((np.minimum(af, 1 - af) >= 0.05) & ((n - ok.sum(axis=1)) / n <= 0.1))
        assert by_codes.tolist() == [1, 3, 5]


def test_neither_node(tmp_path):
    from saigegds_amd.gds_write import GdsWriter
    w = GdsWriter(str(tmp_path / "none.gds"))
    w.put_attr("FileFormat", "SEQ_ARRAY")
    w.add("sample.id", ["a", "b", "c"], "none")
    w.add("variant.id", np.arange(1, 3), "none")
    w.close()
    with pytest.raises(ValueError, match="'genotype' and 'annotation/format/DS' are not available."):
        _markers(str(tmp_path / "none.gds"), ["a", "b", "c"])


def test_both_nodes_take_the_genotypes(tmp_path):
    """A file with genotype/data and a DS node of other values: the genotype route, the DS node is not read."""
    from saigegds_amd.gds_write import GdsWriter
    m, n = 300, 1000
    g = GdsFile(os.path.join(GOLD, "grm1k_10k_snp.gds"))
    assert g.has_genotype() and np.all(np.asarray(g.read("genotype/@data"))[:m] == 1)
    codes, sid = P.golden_codes(m)
    ref = _markers(GenotypeSource(sid, packed=pack_dosage_2bit(codes)), sid, maf=0.05)
    assert 0 < ref["idx"].size < m
    # the first 300 variants' genotypes, and a DS node whose every dosage is 1.0 (maf 0.5: its filter would keep all)
    fn = str(tmp_path / "both.gds")
    w = GdsWriter(fn)
    w.put_attr("FileFormat", "SEQ_ARRAY")
    w.add("sample.id", sid, "none")
    w.add("variant.id", np.arange(1, m + 1), "none")
    w.add("genotype/data", g.raw_range("genotype/data", 0, m * n // 2), "none", cls="dBit2", dims=(m, n, 2))
    w.add("genotype/@data", np.ones(m, dtype="<i4").tobytes(), "none", cls="dInt32", dims=(m,))
    w.add("annotation/format/DS/data", np.full((m, n), 64, dtype=np.uint8), "none", cls="dPackedReal8U", dims=(m, n),
          scale=1 / 64, offset=0.0)
    w.add("annotation/format/DS/@data", np.ones(m, dtype="<i4").tobytes(), "none", cls="dInt32", dims=(m,))
    w.close()
    _same_markers(_markers(fn, sid, maf=0.05), ref)


def _golden_inputs():
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    data = {"sample.id": ph["sample_id"], "y": ph["y"], "x1": ph["x1"], "x2": ph["x2"]}
    return g, data


def test_binary_fit_from_the_dosage_file(tmp_path):
    """The golden hard calls as a dPackedReal8U dosage file: the fit (oracle operator) equals the fit from the
    GenotypeSource of the same codes, array for array."""
    from oracle.oracle import GrmOracle
    g, data = _golden_inputs()
    codes, sid = P.golden_codes(10000)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    fn = P.write_ds_file(tmp_path / "ds_only.gds", P.encode(x, "dPackedReal8U", 1 / 64, 0.0), "dPackedReal8U", 1 / 64, 0.0, sid)
    m = seqFitNullGLMM_SPA("y ~ x1 + x2", data, fn, verbose=False, operator_factory=GrmOracle)
    src = GenotypeSource(list(g["sample_id"]), packed=g["packed"][:10000], variant_id=g["variant_id"][:10000])
    ref = seqFitNullGLMM_SPA("y ~ x1 + x2", data, src, verbose=False, operator_factory=GrmOracle)
    for k in ARRAYS:
        assert np.array_equal(np.asarray(getattr(m, k)), np.asarray(getattr(ref, k))), k
    for k in ref.var_ratio_table:
        assert np.array_equal(np.asarray(m.var_ratio_table[k]), np.asarray(ref.var_ratio_table[k])), k
    assert list(m.sample_id) == list(ref.sample_id) and m.converged == ref.converged


def test_gxg_with_a_dosage_only_grm_file(tmp_path):
    from oracle import GrmOracle
    from saigegds_amd.gxg import seqGLMM_GxG_spa
    g, data = _golden_inputs()
    codes, sid = P.golden_codes(10000)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    fn = P.write_ds_file(tmp_path / "grm_ds.gds", P.encode(x, "dPackedReal8U", 1 / 64, 0.0), "dPackedReal8U", 1 / 64, 0.0, sid)
    src = GenotypeSource(list(g["sample_id"]), packed=g["packed"], variant_id=g["variant_id"])
    pairs = {"a": [2], "b": [6]}
    kw = dict(variant_id=list(range(1, 10001, 20)), verbose=False, operator_factory=lambda p, n: GrmOracle(p, n))
    got = seqGLMM_GxG_spa("y ~ x1 + x2", data, fn, src, pairs, **kw)
    ref = seqGLMM_GxG_spa("y ~ x1 + x2", data, src, src, pairs, **kw)
    assert list(got) == list(ref) and got.nrow == 1
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), k
