"""Aggregate tests on dosage input through the C ABI (sgx_dsblock_*): the collapse kernel against the 2-bit one bit for
bit, the block's scan against the host-buffer scans, the drivers against the restatement of tests/aggregate_ds_ref.py."""
import os

import numpy as np
import pytest

import aggregate_ds_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _model(n):
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    if n == 1000:
        mod = R.golden_model()
        return init_nullmod(mod, np.arange(1000), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    mod = synth.synth_null_model(n, "binary", 0.05, n_cov=3, seed=20260)
    return init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))


def _hard_calls(n, m, seed):
    rng = np.random.default_rng(seed)
    af = 10 ** rng.uniform(-2.3, -0.4, m)
    af[::7] = 1 - af[::7]                                          # alt-major rows: flipped entries
    codes = (rng.random((m, n)) < af[:, None]).astype(np.uint8) + (rng.random((m, n)) < af[:, None]).astype(np.uint8)
    codes[rng.random((m, n)) < 0.01] = 3
    return codes


def _as(codes, dtype):
    if dtype == np.uint8:
        return np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    if dtype == np.int32:
        return np.where(codes == 3, R.NA_INT, codes.astype(np.int64)).astype(np.int32)
    return np.where(codes == 3, np.nan, codes.astype(np.float64))


@pytest.mark.parametrize("n", [1000, 70001])
def test_g1_collapse_of_hard_calls_equals_the_2bit_kernel(n):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    m, per = 48, 8
    codes = _hard_calls(n, m, 11 + n)
    packed = pack_dosage_2bit(codes)
    rng = np.random.default_rng(5)
    ok = codes != 3
    nn = ok.sum(axis=1)
    ss = np.where(ok, codes, 0).sum(axis=1)
    flip = ss > nn
    mean = np.where(flip, 2 - ss / nn, ss / nn)
    grp_ptr = np.arange(0, m + 1, per)
    var_idx = rng.permutation(m).astype(np.int32)                  # entries in an order of their own
    with Scanner(_model(n)) as sc:
        for nc in (1, 4):
            w = rng.random((m, nc)) / per
            if nc > 1:
                w[rng.random((m, nc)) < 0.3] = np.nan              # entry not in that column
            fl, mn = flip[var_idx], mean[var_idx]
            mw = mn[:, None] * w
            # the 2-bit form: one row per (group, column), one table per entry with a finite weight
            row_ptr, vix, lut = [0], [], []
            for g in range(m // per):
                for c in range(nc):
                    for e in range(grp_ptr[g], grp_ptr[g + 1]):
                        if np.isfinite(w[e, c]):
                            vix.append(var_idx[e])
                            lut.append([2 * w[e, c], 1 * w[e, c], 0 * w[e, c], mw[e, c]] if fl[e]
                                       else [0 * w[e, c], 1 * w[e, c], 2 * w[e, c], mw[e, c]])
                    row_ptr.append(len(vix))
            ref, ref_valid = sc.burden_2bit(packed, np.asarray(row_ptr), np.asarray(vix, dtype=np.int32),
                                            np.asarray(lut, dtype=np.float64).reshape(-1, 4))
            assert ref_valid.sum() >= ref_valid.size // 2
            for dtype in (np.uint8, np.int32, np.float64):
                with sc.dosage_block(dtype, m) as blk:
                    nv, sm, st = blk.load(_as(codes, dtype))
                    assert np.array_equal(nv, nn) and np.array_equal(st, ss) and np.array_equal(sm, ss.astype(np.float64))
                    out, valid = blk.burden(grp_ptr, var_idx, fl.astype(np.uint8), w, mw)
                what = f"N={n} {np.dtype(dtype)} {nc} column(s)"
                assert np.array_equal(valid, ref_valid), what
                assert out.tobytes() == ref.tobytes() or np.array_equal(out, ref, equal_nan=True), what


@pytest.mark.parametrize("n", [1000, 70001])
def test_g2_block_scan_equals_host_buffer_scans(n):
    import torch  # noqa: F401
    from conftest import assert_table_close
    from saigegds_amd._lib import Scanner
    m = 64
    codes = _hard_calls(n, m, 3)
    rng = np.random.default_rng(8)
    with Scanner(_model(n)) as sc:
        # fractional / non-hard-call rows: the dosage kernels on both sides, bit for bit
        f64 = _as(codes, np.float64)
        f64 = np.where(np.isnan(f64), np.nan, np.rint(np.clip(f64 + rng.normal(0, 0.1, f64.shape), 0, 2) * 127) / 127)
        u8 = _as(codes, np.uint8)
        u8[:, 0] = 5
        i32 = _as(codes, np.int32)
        i32[:, 0] = 5
        for ds, host in ((f64, sc.scan_f64), (u8, sc.scan_u8), (i32, sc.scan_i32)):
            ref, ref_valid = host(ds)
            with sc.dosage_block(ds.dtype, m) as blk:
                nv, sm, st = blk.load(ds)
                out, valid = blk.scan()
            what = f"N={n} {ds.dtype}"
            assert np.array_equal(valid, ref_valid) and np.array_equal(out, ref, equal_nan=True), what
            ok = R.ok_mask(ds)
            z = np.where(ok, ds, 0)
            assert np.array_equal(nv, ok.sum(axis=1)), what
            assert np.array_equal(st, np.floor(z).astype(np.int64).sum(axis=1)), what
            plain = z.astype(np.float64).sum(axis=1)
            print(what, "max rel. error of sum", np.max(np.abs(sm - plain) / np.maximum(plain, 1e-300)))
            assert np.all(np.abs(sm - plain) <= 1e-14 * np.abs(plain)), what
        # hard calls: the host-buffer scans pack them to 2-bit; the block keeps the dosage kernels
        for dtype in (np.uint8, np.int32):
            ds = _as(codes, dtype)
            ref, ref_valid = (sc.scan_u8 if dtype == np.uint8 else sc.scan_i32)(ds)
            with sc.dosage_block(dtype, m) as blk:
                blk.load(ds)
                out, valid = blk.scan()
            assert_table_close(out, valid, ref, ref_valid, what=f"N={n} hard calls {np.dtype(dtype)}")


def test_g2_i32_block_loads_in_three_chunks():
    """N = 1000, 600 int32 rows that are not all hard calls: pipe_mb = 1 is 262 rows of 4000 bytes, so the load cuts
    chunks of 262, 262 and 76, the third into the pipeline buffer of the first.  Counts and table equal those of the
    one-chunk load, and the table equals sgx_scan_i32 of the same rows at the same pipe_mb, all bit for bit."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    n, m = 1000, 600
    i32 = _as(_hard_calls(n, m, 6), np.int32)
    i32[:, 0] = 5
    assert m > 2 * ((1 << 20) // (4 * n))
    got = {}
    with Scanner(_model(n)) as sc:
        try:
            for pipe_mb in (0, 1):
                sc.set_option("pipe_mb", pipe_mb)
                with sc.dosage_block(np.int32, m) as blk:
                    nv, sm, st = blk.load(i32)
                    out, valid = blk.scan()
                ref, ref_valid = sc.scan_i32(i32)
                print("pipe_mb", pipe_mb, "valid", int(valid.sum()))
                assert np.array_equal(valid, ref_valid) and np.array_equal(out, ref, equal_nan=True), pipe_mb
                got[pipe_mb] = (nv, sm, st, out, valid)
        finally:
            sc.set_option("pipe_mb", 0)
    assert got[0][4].sum() > m // 2
    for a, b, what in zip(got[1], got[0], ("n_valid", "sum", "sum_trunc", "table", "valid")):
        assert np.array_equal(a, b, equal_nan=(what in ("sum", "table"))), what


def test_g3_c1_gds_file_on_the_device():
    import torch  # noqa: F401
    mod = R.golden_model()
    path, ds, sid, units = R.case_c1()
    b, v, o = R.run_drivers(path, mod, units, dsnode="")
    R.check_against_restatement(b, v, o, ds, units, R.oracle_for(mod, sid), "G3 / C1")


def test_g3_c2_fractional_f64_in_batches_on_the_device():
    import torch  # noqa: F401
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    x, sid, units = R.case_c2()
    src = GenotypeSource(sid, dosage=x)
    b, v, o = R.run_drivers(src, mod, units, ds_budget=40 * 8000)
    R.check_against_restatement(b, v, o, x, units, R.oracle_for(mod, sid), "G3 / C2")
    b2, v2, o2 = R.run_drivers(src, mod, units, ds_budget=1 << 40)
    R.same_dicts(b, b2, "G3 / C2 burden, batches vs one batch")
    R.same_dicts(v, v2, "G3 / C2 ACAT-V, batches vs one batch")
    R.same_dicts(o, o2, "G3 / C2 ACAT-O, batches vs one batch")


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_g3_integer_dosages_on_the_device(dtype):
    import torch  # noqa: F401
    from saigegds_amd.assoc import GenotypeSource
    mod = R.golden_model()
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    from saigegds_amd.gds import unpack_dosage_2bit
    codes = unpack_dosage_2bit(g["packed"][:60], 1000).astype(np.int64)
    miss = codes == 3
    for j in (3, 22):
        codes[j] = np.where(miss[j], 3, 2 - codes[j])
    ds = np.where(miss, 0xFF if dtype == np.uint8 else R.NA_INT, codes).astype(dtype)
    ds[7, 5] = 3
    sid = [str(s) for s in g["sample_id"]]
    units = [np.arange(s, s + 15) + 1 for s in range(0, 60, 15)]
    b, v, o = R.run_drivers(GenotypeSource(sid, dosage=ds), mod, units)
    R.check_against_restatement(b, v, o, ds, units, R.oracle_for(mod, sid), f"G3 integer {np.dtype(dtype)}",
                                need_spa=False, integer_input=True)


def test_g3_c4_truncated_sum_on_the_device():
    import torch  # noqa: F401
    from saigegds_amd.assoc import GenotypeSource
    from test_aggregate_dosage import c4_case
    mod = R.golden_model()
    x, sid, units = c4_case()
    b, v, o = R.run_drivers(GenotypeSource(sid, dosage=x), mod, units)
    R.check_against_restatement(b, v, o, x, units, R.oracle_for(mod, sid), "G3 / C4", need_spa=False)


def test_g4_large_n_every_row_against_the_restatement():
    """N = 430 000, f64 fractional dosages, 0.5 % missing, 6 units of 8 variants, 4 columns (two weight sets: all
    variants and the rare ones)."""
    import torch  # noqa: F401
    from oracle.oracle import Oracle
    from saigegds_amd._lib import Scanner
    from saigegds_amd.aggregate import AggrParamBeta as wb
    n, nu, per = 430000, 6, 8
    sm = _model(n)
    rng = np.random.default_rng(430)
    m = nu * per
    x = np.empty((m, n))
    for j in range(m):
        af = 10 ** rng.uniform(-3.5, -1.0)
        if j % 11 == 5:
            af = 1 - af
        g = (rng.random(n) < af).astype(np.float64) + (rng.random(n) < af)
        g = np.clip(g + rng.normal(0, 0.05, n) * (g > 0), 0, 2)
        x[j] = np.rint(g * 127) / 127
        x[j, rng.random(n) < 0.005] = np.nan
    orc = Oracle(sm)
    with Scanner(sm) as sc, sc.dosage_block(np.float64, m) as blk:
        nv, s, st = blk.load(x)
        nvf = nv.astype(np.float64)
        af = s / (2 * nvf)
        maf, mac = np.minimum(af, 1 - af), np.minimum(s, 2 * nvf - s)
        rmaf, rmac = R.ds_mat_mafmac(x)
        R.close(maf, rmaf, "G4 maf")
        R.close(mac, rmac, "G4 mac")
        assert np.array_equal(st, [R.trunc_sum(r) for r in x])
        cols = []
        for u in range(nu):
            r = slice(u * per, (u + 1) * per)
            cu = [R.normalize([R.dbeta(p, a, b) for p in rmaf[r]]) for a, b in wb.T]
            cu += [R.normalize([R.dbeta(p, a, b) if c < 200 else np.nan for p, c in zip(rmaf[r], rmac[r])]) for a, b in wb.T]
            cols.append(np.array(cu).T)
        w = np.concatenate(cols)
        flip = st > nv
        mean = np.where(flip, 2 - st / nvf, st / nvf)
        out, valid = blk.burden(np.arange(0, m + 1, per), np.arange(m, dtype=np.int32), flip.astype(np.uint8), w, mean[:, None] * w)
    rows = np.stack([R.ds_mat_burden(x[u * per:(u + 1) * per], w[u * per:(u + 1) * per, c], list(st[u * per:(u + 1) * per]))
                     for u in range(nu) for c in range(4)])
    ref, ref_valid = orc.scan_f64(rows)
    assert np.array_equal(valid, ref_valid) and ref_valid.sum() >= 12
    for k in range(nu * 4):
        if ref_valid[k]:
            R.close(out[k, :7], ref[k, :7], f"G4 row {k}")
            assert out[k, 7] == ref[k, 7]


def test_g5_error_paths_leave_the_handle_usable():
    import ctypes as C
    import torch  # noqa: F401
    from saigegds_amd import _lib
    from saigegds_amd._lib import Scanner, SgxError
    L = _lib.load()
    codes = _hard_calls(1000, 16, 2)
    ds = _as(codes, np.float64)
    with Scanner(_model(1000)) as sc:
        b = C.c_void_p()
        assert L.sgx_dsblock_create(1000, 7, 4, 0, C.byref(b)) == -1 and b"dtype" in L.sgx_last_error()
        assert L.sgx_dsblock_create(0, 2, 4, 0, C.byref(b)) == -1
        with sc.dosage_block(np.float64, 16) as blk:
            nv = np.empty(16, dtype=np.int32)
            assert L.sgx_dsblock_load(sc._h, blk._b, None, 16, nv.ctypes.data, None, None) == -1 and L.sgx_last_error()
            assert L.sgx_dsblock_scan(sc._h, blk._b, None, None) == -1
            with pytest.raises(SgxError, match="holds up to"):
                blk.load(np.concatenate([ds, ds]))
            with pytest.raises(SgxError, match="nothing loaded"):
                blk.scan()
            blk.load(ds)
            w = np.full((4, 2), 0.25)
            ok = (np.array([0, 4]), np.arange(4, dtype=np.int32), np.zeros(4, dtype=np.uint8), w, w)
            for bad, msg in (((np.array([0, 4]), np.array([0, 1, 2, 16], dtype=np.int32)) + ok[2:], "outside the block"),
                             ((np.array([0, 5, 4]), np.arange(4, dtype=np.int32)) + ok[2:], "not ascending"),
                             (ok[:3] + (np.full((4, 65), 0.25), np.full((4, 65), 0.25)), "n_cols")):
                with pytest.raises(SgxError, match=msg) as ei:
                    blk.burden(*bad)
                assert ei.value.code == -1
            with sc.dosage_block(np.uint8, 4) as other, Scanner(_model(70001)) as sc2:
                with pytest.raises(SgxError, match="Invalid length of dosages"):
                    C_rc = L.sgx_dsblock_scan(sc2._h, other._b, np.empty(8).ctypes.data, np.empty(1, dtype=np.uint8).ctypes.data)
                    _lib.check(C_rc)
            out, valid = blk.burden(*ok)
            ref, ref_valid = blk.scan()
        assert valid.shape == (2,) and ref_valid.shape == (16,)
        out2, valid2 = sc.scan_f64(ds)                            # the handle still works
        assert np.array_equal(valid2, ref_valid) and np.array_equal(out2, ref, equal_nan=True)
