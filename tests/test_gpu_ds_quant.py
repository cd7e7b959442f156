"""Stored dosage rows -> 2-bit hard-call rows and the marker filter's counts on the device (sgx_quantize_packed), against
the numpy statement of the rule in ds_quant_cases; the null-model fit on a file that holds only dosages."""
import ctypes as C
import os

import numpy as np
import pytest

import ds_quant_cases as Q
import packed_ds_cases as P
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 1000, 4099]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _check(got, raw, cls, scale, offset, sel, n, what):
    """Packed bytes and the three integer counts exactly; ds_sum exactly for the integer classes (dyadic scales: every
    sum exact), float32 within 4 n 2^-53 sum|v|: the worst case of reordering a double sum of n terms."""
    pk, nv, sm, dv, ds = got
    r_pk, r_nv, r_sm, r_dv, r_ds, r_abs = Q.ref_quantize(raw, cls, scale, offset, sel)
    err = np.abs(ds - r_ds)
    bound = 4.0 * n * 2.0 ** -53 * r_abs if cls == "dFloat32" else np.zeros_like(r_abs)
    print(what, "rows", raw.shape[0], "bytes that differ", int((pk != r_pk).sum()), "max ds_sum error", float(err.max()),
          "max bound", float(bound.max()))
    assert pk.shape == r_pk.shape and pk.dtype == np.uint8
    assert np.array_equal(pk, r_pk), what
    assert np.array_equal(nv, r_nv) and np.array_equal(sm, r_sm) and np.array_equal(dv, r_dv), what
    assert np.all(err <= bound), what


@pytest.mark.parametrize("mode", ["all", "sel", "sel_odd"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_q1_parity(cls, n, mode):
    """Every class and size: the file's samples as they are (rows n values apart: with an odd n, and at n = 1000 of one
    byte, they start off the 16-byte lines), a permuted selection out of n + 37, and out of an odd number of samples."""
    from saigegds_amd._lib import quantize_packed
    raw, scale, offset, where = Q.parity_rows(cls, n, seed=1000 + n)
    sel = None
    if mode != "all":
        n_file = n + 37
        n_file += (mode == "sel_odd" and n_file % 2 == 0)
        raw, sel = P.widen(raw, n_file, seed=n)
        assert mode == "sel" or raw.shape[1] % 2 == 1
    got = quantize_packed(raw, cls, scale, offset, n, sel=sel)
    # the edge values' codes, stated one by one
    codes = np.stack([(got[0] >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(raw.shape[0], -1)
    for r, c, code in where:
        assert codes[r, c] == code, (cls, n, mode, r, c)
    _check(got, raw, cls, scale, offset, sel, n, f"{cls} n={n} {mode}")


@pytest.mark.parametrize("cls", ["dPackedReal8U", "dFloat32"])
def test_q2_many_rows(cls):
    """70 000 rows of 5 samples: more rows than grid.y holds.  Exact (values on the grid of 2^-6 / 2^-14)."""
    from saigegds_amd._lib import quantize_packed
    rng = np.random.default_rng(5)
    scale, offset = P.DYADIC[cls]
    if cls == "dFloat32":
        raw = (rng.integers(-8192, 49152, (70000, 5)) / 16384).astype(np.float32)
        raw[rng.random(raw.shape) < 0.02] = np.nan
    else:
        raw = rng.integers(0, 256, (70000, 5), dtype=np.uint8)
    pk, nv, sm, dv, ds = quantize_packed(raw, cls, scale, offset, 5)
    r = Q.ref_quantize(raw, cls, scale, offset)
    assert np.array_equal(pk, r[0]) and np.array_equal(nv, r[1]) and np.array_equal(sm, r[2]) and np.array_equal(dv, r[3])
    assert np.array_equal(ds, r[4])


@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("cls", ["dPackedReal16U", "dFloat32"])
def test_q3_chunks(cls, with_sel):
    """300 rows of 1000 samples in one chunk, a row a chunk and seven rows a chunk (42 chunks and a tail of six): all
    five outputs identical -- float32 dosages that are no dyadic grid, so their sum does depend on the order -- and
    identical from call to call."""
    from saigegds_amd._lib import quantize_packed
    rng = np.random.default_rng(9)
    _, _, scale, offset = P.CLASSES[cls]
    x = P.dosages(300, 1000, 77)
    raw = P.stored_rows(cls, x + (rng.random(x.shape) * 1e-3 if cls == "dFloat32" else 0.0))
    sel = None
    if with_sel:
        raw, sel = P.widen(raw, 1037, seed=3)
    row = raw.shape[1] * raw.dtype.itemsize
    first = quantize_packed(raw, cls, scale, offset, 1000, sel=sel, chunk_bytes=0)
    _check(first, raw, cls, scale, offset, sel, 1000, f"{cls} chunks")
    for cb in (0, row, 7 * row):
        again = quantize_packed(raw, cls, scale, offset, 1000, sel=sel, chunk_bytes=cb)
        for a, b in zip(first, again):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (cls, with_sel, cb)


def test_q4_bad_arguments():
    """Every refused argument returns SGX_EINVAL and leaves the output buffers as they were; a valid call then works."""
    from saigegds_amd import _lib
    L = _lib.load()
    n, nfs, m = 40, 50, 6
    raw = np.random.default_rng(2).integers(0, 255, (m, nfs), dtype=np.uint8)
    same = np.ascontiguousarray(raw[:, :n])
    sel = np.arange(n, dtype=np.int32)[::-1].copy()
    bad_hi, bad_lo = sel.copy(), sel.copy()
    bad_hi[7], bad_lo[n - 1] = nfs, -1
    nb = (n + 3) // 4
    pk = np.full((m, nb), 0xA5, dtype=np.uint8)
    cnt = [np.full(m, -77, dtype=np.int32) for _ in range(3)]
    ds = np.full(m, -77.5)

    def call(raw_p=raw.ctypes.data, cls=0, nfs_=nfs, sel_p=sel.ctypes.data, n_=n, m_=m, pk_p=pk.ctypes.data, stride=nb,
             c0=cnt[0].ctypes.data, c1=cnt[1].ctypes.data, c2=cnt[2].ctypes.data, d=ds.ctypes.data):
        return L.sgx_quantize_packed(raw_p, cls, nfs_, 1 / 64, 0.0, sel_p, n_, m_, 0, 0, pk_p, stride, c0, c1, c2, d)

    bad = {"class 5": dict(cls=5), "class -1": dict(cls=-1), "NULL raw": dict(raw_p=None), "NULL packed_out": dict(pk_p=None),
           "NULL n_valid": dict(c0=None), "NULL allele_sum": dict(c1=None), "NULL ds_valid": dict(c2=None),
           "NULL ds_sum": dict(d=None), "n_samp 0": dict(n_=0), "n_samp -1": dict(n_=-1),
           "n_file_samp < n_samp": dict(nfs_=n - 1), "no sel, n_file_samp != n_samp": dict(sel_p=None),
           "index == n_file_samp": dict(sel_p=bad_hi.ctypes.data), "index -1": dict(sel_p=bad_lo.ctypes.data),
           "out_stride": dict(stride=nb - 1)}
    for what, kw in bad.items():
        assert call(**kw) == -1, what                    # SGX_EINVAL
        assert np.all(pk == 0xA5) and all(np.all(c == -77) for c in cnt) and np.all(ds == -77.5), what
    assert call(m_=0) == 0                               # no rows: nothing to do, nothing written
    assert np.all(pk == 0xA5) and np.all(ds == -77.5)
    assert call() == 0
    got = (pk, cnt[0], cnt[1], cnt[2], ds)
    _check(got, raw, "dPackedReal8U", 1 / 64, 0.0, sel, n, "after the refused calls")
    assert call(raw_p=same.ctypes.data, nfs_=n, sel_p=None) == 0
    _check(got, same, "dPackedReal8U", 1 / 64, 0.0, None, n, "no selection")


# ---------------------------------------------------------------------------
# the fit, end to end

TOL = 1e-4          # the reference's checkEquals(mod, glmm, tolerance=1e-4), as tests/test_fitnull.py states it

ARRAYS = ("tau", "coefficients", "fitted_values", "linear_predictors", "residuals", "cov", "y", "V", "X1", "XV",
          "XXVX_inv", "mu_noK", "res_noK", "var_ratio", "variant_id")


def _mean_rel(a, b):
    """R's all.equal.numeric: sum|a-b| / sum|b| (absolute when the target is ~0)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape
    xy, xn = np.sum(np.abs(a - b)), np.sum(np.abs(b))
    return xy / xn if xn > 1e-300 else xy


def _check_model(m, gold, tol=TOL):
    """The comparison of tests/test_fitnull.py with a golden model, restated."""
    assert m.trait_type == str(gold["trait_type"])
    assert list(m.sample_id) == list(gold["sample_id"])
    assert np.array_equal(np.asarray(m.variant_id), gold["variant_id"])
    assert bool(m.converged) == bool(gold["converged"])
    for name, val in [("tau", m.tau), ("coefficients", m.coefficients), ("fitted_values", m.fitted_values),
                      ("linear_predictors", m.linear_predictors), ("residuals", m.residuals), ("cov", m.cov),
                      ("y", m.y), ("V", m.V), ("X1", m.X1), ("XV", m.XV), ("XXVX_inv", m.XXVX_inv),
                      ("noK_mu", m.mu_noK), ("noK_res", m.res_noK)]:
        assert _mean_rel(val, gold[name]) < tol, name
    assert np.array_equal(np.asarray(m.var_ratio_table["id"], dtype=np.int64), gold["vr_id"].astype(np.int64))
    for k in ("maf", "mac", "var1", "var2", "ratio"):
        assert _mean_rel(m.var_ratio_table[k], gold["vr_" + k]) < tol, k


def test_q5_fit_from_a_dosage_only_file(tmp_path):
    """The golden hard calls written as dPackedReal8U dosages (scale 1/64, ZIP_RA) into a file without a genotype node:
    the fit on that file equals the fit from the golden GenotypeSource array for array -- same codes and exact counts
    give the same kept markers and the same operator -- and passes the comparison with the reference's model."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.fitnull import seqFitNullGLMM_SPA
    codes, sample_id = P.golden_codes(10000)
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    ph = np.load(os.path.join(GOLDEN, "pheno.npz"))
    data = {"sample.id": ph["sample_id"], "y": ph["y"], "x1": ph["x1"], "x2": ph["x2"]}
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    fn = P.write_ds_file(tmp_path / "ds_only.gds", P.encode(x, "dPackedReal8U", 1 / 64, 0.0), "dPackedReal8U", 1 / 64, 0.0,
                         sample_id)
    m = seqFitNullGLMM_SPA("y ~ x1 + x2", data, fn, verbose=False)
    src = GenotypeSource(list(g["sample_id"]), packed=g["packed"][:10000], variant_id=g["variant_id"][:10000])
    ref = seqFitNullGLMM_SPA("y ~ x1 + x2", data, src, verbose=False)
    for k in ARRAYS:
        assert np.array_equal(np.asarray(getattr(m, k)), np.asarray(getattr(ref, k))), k
    for k in ref.var_ratio_table:
        assert np.array_equal(np.asarray(m.var_ratio_table[k]), np.asarray(ref.var_ratio_table[k])), k
    assert list(m.sample_id) == list(ref.sample_id) and m.converged == ref.converged
    _check_model(m, np.load(os.path.join(GOLDEN, "saige_model.npz")))
