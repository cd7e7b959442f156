"""Aggregate tests on dosage input (INTSXP / REALSXP branches of ds_mat_mafmac / ds_mat_burden): the driver's host
logic -- node resolution, batching, weights, flip / mean tables, combination -- with the numpy scanner of
tests/aggregate_ds_ref.py in place of the library, against the restatement there (no GPU needed).  The same cases run
on the device in tests/test_gpu_aggregate_dosage.py."""
import os

import numpy as np
import pytest

import aggregate_ds_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KW = {"scanner_factory": R.NumpyDsScanner}


def test_c1_gds_file_without_genotype_node():
    """assoc_100snp.gds has no genotype/data: dsnode = "" resolves to annotation/format/DS (path given as a string)."""
    mod = R.golden_model()
    path, ds, sid, units = R.case_c1()
    b, v, o = R.run_drivers(path, mod, units, dsnode="", **KW)
    R.check_against_restatement(b, v, o, ds, units, R.oracle_for(mod, sid), "C1")
    assert R.NumpyDsScanner.last.uploads == 1                      # 100 rows of 8 000 bytes: one batch, one upload


def test_c2_fractional_f64_in_batches():
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    x, sid, units = R.case_c2()
    assert np.isnan(x[17]).all() and np.nanmax(x[30]) == 0 and np.any(np.nansum(x, axis=1) > 1000)
    src = GenotypeSource(sid, dosage=x)
    b, v, o = R.run_drivers(src, mod, units, ds_budget=40 * 8000, **KW)       # 40 rows of 8 000 bytes per batch
    assert R.NumpyDsScanner.last.uploads >= 3
    R.check_against_restatement(b, v, o, x, units, R.oracle_for(mod, sid), "C2")
    b2, v2, o2 = R.run_drivers(src, mod, units, ds_budget=1 << 40, **KW)
    assert R.NumpyDsScanner.last.uploads == 1
    R.same_dicts(b, b2, "C2 burden, batches vs one batch")
    R.same_dicts(v, v2, "C2 ACAT-V, batches vs one batch")
    R.same_dicts(o, o2, "C2 ACAT-O, batches vs one batch")


def test_c2_samples_selected_and_reordered():
    """The source holds more samples than the model, in another order: rows are cut to the model's samples."""
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    x, sid, units = R.case_c2(n_var=48)
    rng = np.random.default_rng(1)
    perm = rng.permutation(1000)
    x2 = np.concatenate([x[:, perm], rng.random((48, 7))], axis=1)
    sid2 = [sid[i] for i in perm] + [f"extra{k}" for k in range(7)]
    b, v, o = R.run_drivers(GenotypeSource(sid2, dosage=x2), mod, units, **KW)
    R.check_against_restatement(b, v, o, x[:, perm], units, R.oracle_for(mod, [sid[i] for i in perm]), "C2 reordered",
                                need_spa=False)


def test_c3_hard_calls_take_the_2bit_path():
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    mod = R.golden_model()
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    packed = g["packed"][:120]
    codes = unpack_dosage_2bit(packed, 1000)
    sid = [str(s) for s in g["sample_id"]]
    units = [np.arange(s, s + 20) + 1 for s in range(0, 120, 20)]
    u8 = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    i32 = np.where(codes == 3, R.NA_INT, codes.astype(np.int64)).astype(np.int32)
    res = [R.run_drivers(GenotypeSource(sid, **kw), mod, units, **KW)
           for kw in ({"packed": packed}, {"dosage": u8}, {"dosage": i32})]
    assert R.NumpyDsScanner.last.uploads == 0                      # no dosage block: the shortcut
    for other, nm in ((res[1], "uint8"), (res[2], "int32")):
        for a, c, what in zip(res[0], other, ("burden", "ACAT-V", "ACAT-O")):
            R.same_dicts(a, c, f"C3 {nm} {what}")


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_integer_dosages_that_are_not_hard_calls(dtype):
    """One value outside 0 / 1 / 2 sends an integer matrix through the dosage block (INTSXP / RAW arithmetic:
    integer sums, 2 - s[j] in integers); integer-valued columns exact."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    mod = R.golden_model()
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:60], 1000).astype(np.int64)
    miss = codes == 3
    for j in (3, 22):
        codes[j] = np.where(miss[j], 3, 2 - codes[j])            # alt-major: the flip branch
    codes[7, 5] = 3 if not miss[7, 5] else codes[7, 5]
    ds = np.where(miss, 0xFF if dtype == np.uint8 else R.NA_INT, codes).astype(dtype)
    ds[7, 5] = 3                                                  # a dosage of 3: not a hard call
    sid = [str(s) for s in g["sample_id"]]
    units = [np.arange(s, s + 15) + 1 for s in range(0, 60, 15)]
    b, v, o = R.run_drivers(GenotypeSource(sid, dosage=ds), mod, units, **KW)
    assert R.NumpyDsScanner.last.uploads == 1
    R.check_against_restatement(b, v, o, ds, units, R.oracle_for(mod, sid), f"integer {np.dtype(dtype)}",
                                need_spa=False, integer_input=True)


def c4_case():
    """Variants whose `int sum` (sum of floors) and plain sum decide differently: every present dosage in [1.2, 1.95]
    (plain sum > n: a plain mean would flip; floors sum to n: no flip, imputed mean 1) or in [0.5, 0.98] (floors sum
    to 0: imputed mean 0 instead of about 0.74), some samples missing so that the imputed mean enters the rows.  The
    dosages vary over the samples: a constant row is collinear with the intercept and its single-variant test is 0 / 0."""
    x, sid, units = R.case_c2(n_var=36, win=6)
    rng = np.random.default_rng(4)
    for j, (lo, hi) in ((2, (1.2, 1.95)), (9, (0.5, 0.98)), (20, (1.2, 1.95)), (27, (0.5, 0.98))):
        x[j] = np.where(np.isnan(x[j]), np.nan, np.rint(rng.uniform(lo, hi, 1000) * 127) / 127)
        x[j, 100:130] = np.nan
    return x, sid, units


def test_c4_truncated_sum_decides_flip_and_mean():
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    x, sid, units = c4_case()
    # the quirk bites on this data: plain and truncated sums give different rows
    row = x[2]
    n, plain, tr = int(np.isfinite(row).sum()), float(np.nansum(row)), R.trunc_sum(row)
    assert plain > n and tr <= n and tr == n                       # flip decisions differ
    assert R.trunc_sum(x[9]) == 0 and np.nansum(x[9]) > 0.5 * np.isfinite(x[9]).sum()   # means differ
    w = np.ones(6) / 6
    assert not np.array_equal(R.ds_mat_burden(x[:6], w), R.ds_mat_burden(x[:6], w, [np.nansum(r) for r in x[:6]]))
    b, v, o = R.run_drivers(GenotypeSource(sid, dosage=x), mod, units, **KW)
    R.check_against_restatement(b, v, o, x, units, R.oracle_for(mod, sid), "C4", need_spa=False)


def test_quantitative_burden_works_and_acat_raises():
    from conftest import load_null_model
    from saigegds_amd.aggregate import seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaACAT_V, seqAssocGLMM_spaBurden
    from saigegds_amd.assoc import GenotypeSource
    mod = load_null_model("saige_model_quant.npz")
    x, sid, units = R.case_c2(n_var=24)
    src = GenotypeSource(sid, dosage=x)
    b = seqAssocGLMM_spaBurden(src, mod, units, verbose=False, **KW)
    assert np.isfinite(b["pval.b1_1"]).sum() >= 1 and "p.norm.b1_1" not in b
    for fn in (seqAssocGLMM_spaACAT_V, seqAssocGLMM_spaACAT_O):
        with pytest.raises(NotImplementedError, match="not implemented"):
            fn(src, mod, units, verbose=False, **KW)


def test_unsupported_dosage_type_is_an_error():
    from saigegds_amd.aggregate import seqAssocGLMM_spaBurden
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    x, sid, units = R.case_c2(n_var=24)
    with pytest.raises(TypeError, match="uint8, int32 or float64"):
        seqAssocGLMM_spaBurden(GenotypeSource(sid, dosage=x.astype(np.float32)), mod, units, verbose=False, **KW)


def test_abi_declares_and_binds_the_dosage_block_calls():
    import re
    from saigegds_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "saigehip.h")).read()
    names = set(re.findall(r"\b(sgx_dsblock_\w+)\s*\(", hdr))
    assert names == {"sgx_dsblock_create", "sgx_dsblock_free", "sgx_dsblock_load", "sgx_dsblock_scan", "sgx_dsblock_burden"}
    assert names <= set(_lib.EXPORTS)
