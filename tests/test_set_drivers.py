"""The set-test drivers' one batch loop (saigegds_amd/aggregate.py: ``_prepare``, ``_run``) on its two rows backends, and
the helpers every driver shares: ``dosage_tables``, ``reduce_hard_calls``.  No GPU: the scan oracle stands in for the
library (``NumpyDsScanner``: ``OracleScanner`` plus a dosage block in numpy).

The SKAT driver's cross-route case is tests/test_skat_dosage.py::test_hard_calls_as_float64_equal_the_2bit_driver."""
import dataclasses
import functools
import os

import numpy as np

from aggregate_ds_ref import NumpyDsScanner, case_c1, close, golden_model, run_drivers

GOLD = os.path.join(os.path.dirname(__file__), "golden")
UNITS = [np.arange(s, s + 20) + 1 for s in range(0, 120, 20)]      # the first 120 golden variants, six units of 20
BUDGET = 50 * 8000                                                 # resident float64 rows of 1000 samples: 50


@functools.lru_cache(maxsize=None)
def both_routes():
    """(packed source, the same hard calls as a float64 source with NaN for missing)."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    sid = [str(s) for s in g["sample_id"]]
    codes = unpack_dosage_2bit(g["packed"][:120], 1000)
    return GenotypeSource(sid, packed=g["packed"][:120]), GenotypeSource(sid, dosage=np.where(codes == 3, np.nan, codes.astype(np.float64)))


def test_hard_calls_give_the_same_tables_on_both_routes():
    packed, real = both_routes()
    mod = golden_model()
    a = run_drivers(packed, mod, UNITS, scanner_factory=NumpyDsScanner)
    assert NumpyDsScanner.last.uploads == 0                         # the 2-bit backend: no dosage block
    b = run_drivers(real, mod, UNITS, scanner_factory=NumpyDsScanner, ds_budget=BUDGET)
    assert NumpyDsScanner.last.uploads >= 2                         # the dosage backend, in several batches
    for name, x, y in zip(("burden", "ACAT-V", "ACAT-O"), a, b):
        assert list(x) == list(y), name
        for k in x:
            close(x[k], y[k], f"{name} {k}")
    assert np.isfinite(a[0]["pval.b1_1"]).all() and np.isfinite(a[0]["pval.b1_25"]).all() and np.isfinite(a[2]["pval"]).all()


def test_dosage_tables():
    from saigegds_amd.aggregate import dosage_tables, flip_mean
    n, s = np.array([10.0, 10.0, 8.0, 4.0]), np.array([3.0, 17.0, 8.0, 6.5])      # s > n: flipped
    flip, mean = flip_mean(n, s)
    assert flip.tolist() == [0, 1, 0, 1]
    m = s / n
    lit = np.array([[0, 1, 2, m[0]], [2, 1, 0, 2 - m[1]], [0, 1, 2, m[2]], [2, 1, 0, 2 - m[3]]])
    assert np.array_equal(dosage_tables(flip, mean), lit)
    w = np.array([0.5, 0.25, 3.0, 0.0])
    assert np.array_equal(dosage_tables(flip, mean, w), lit * w[:, None])
    assert dosage_tables(flip[:0], mean[:0]).shape == (0, 4) and dosage_tables(flip, mean).dtype == np.float64


def test_reduce_hard_calls():
    from saigegds_amd.assoc import GenotypeSource, open_scan_input
    from saigegds_amd.aggregate import reduce_hard_calls
    from saigegds_amd.gds import unpack_dosage_2bit
    mod = golden_model()
    sid = both_routes()[0].sample_id()
    codes = np.random.default_rng(5).integers(0, 4, (7, 1000))          # 3 = missing
    for dtype, miss in ((np.uint8, 0xFF), (np.int32, np.iinfo(np.int32).min)):
        ds = np.where(codes == 3, miss, codes).astype(dtype)
        inp = reduce_hard_calls(open_scan_input(GenotypeSource(sid, dosage=ds), mod, "", False))
        assert inp.kind == "packed" and inp.ds_all is None and inp.ds_dtype is None
        assert np.array_equal(unpack_dosage_2bit(inp.packed, 1000), codes)
        ds[2, 5] = 3                                                    # one value that is no hard call
        raw = open_scan_input(GenotypeSource(sid, dosage=ds), mod, "", False)
        assert reduce_hard_calls(raw) is raw and raw.kind == "dosage"
    real = open_scan_input(GenotypeSource(sid, dosage=np.where(codes == 3, np.nan, codes.astype(np.float64))), mod, "", False)
    assert reduce_hard_calls(real) is real and real.kind == "dosage"
    two_bit = open_scan_input(both_routes()[0], mod, "", False)
    assert reduce_hard_calls(two_bit) is two_bit
    path, _, _, _ = case_c1()                                           # a file's dosage node
    backed = open_scan_input(path, mod, "", False)
    assert not backed.in_mem and reduce_hard_calls(backed) is backed and backed.kind != "packed"


def test_prepared_has_no_route_only_fields():
    from saigegds_amd.aggregate import AggrParamBeta, _prepare, _run
    filled = []
    for src in both_routes():
        pr = _prepare(src, golden_model(), UNITS, AggrParamBeta, 0.05, float("nan"), False, "SAIGE burden analysis:", NumpyDsScanner,
                      ds_budget=BUDGET)
        try:
            _run(pr, ("all",))
        finally:
            pr.sc.close()
        filled.append({f.name for f in dataclasses.fields(pr) if getattr(pr, f.name) is not None})
        assert pr.burden["all"][0].shape == (6, 2, 8) and pr.out.shape == (120, 8) and pr.skat is None
    assert filled[0] == filled[1] and {"index", "n", "s", "maf", "mac", "pval", "out", "valid", "burden"} <= filled[0]
