"""Packed-real dosage rows through the C ABI as the file stores them (sgx_scan_packed, sgx_ds_block_load_packed): decoded
and sample-selected on the device, against the float64 calls on the host-decoded rows bit for bit, and against the
oracle; the drivers on files with such a node."""
import os

import numpy as np
import pytest

import packed_ds_cases as P
from conftest import GOLDEN, assert_table_close, scan_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _same(a, b):
    """np.array_equal with NaN == NaN (tests/test_gpu_baseline.py:259)."""
    return a.shape == b.shape and np.array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0))


def _check_scan(sc, raw, cls, scale, offset, sel, what, orc=None, quant=False, exact_sums=True):
    """scan_packed == scan_f64(decoded[:, sel]) bit for bit (and the oracle within the scan's tolerance)."""
    dec = P.decode(raw, cls, scale, offset)
    dec = np.ascontiguousarray(dec if sel is None else dec[:, sel])
    ref, ref_valid = sc.scan_f64(dec)
    out, valid = sc.scan_packed(raw, cls, scale, offset, sel)
    print(what, "rows", raw.shape[0], "valid", int(ref_valid.sum()), "rows that differ",
          int((~np.all(np.nan_to_num(out, nan=-7.0) == np.nan_to_num(ref, nan=-7.0), axis=1)).sum()))
    assert np.array_equal(valid, ref_valid), what
    assert _same(out, ref), what
    if orc is not None:
        o_ref, o_valid = orc.scan_f64(dec)
        if not exact_sums:
            # AF, mac, num of rows whose sums round differ from the oracle's sample-by-sample sums by the order of the
            # additions only (tests/test_gpu_baseline.py::test_baseline_c3_real_dosages): 1e-9 there, the rest as usual
            assert np.array_equal(valid, o_valid), what
            v = o_valid.astype(bool)
            np.testing.assert_allclose(out[v][:, :3], o_ref[v][:, :3], rtol=1e-9, err_msg=what)
            out = out.copy()
            out[:, :3] = o_ref[:, :3]
        assert_table_close(out, valid, o_ref, o_valid, quant=quant, what=what)
    return out, valid


@pytest.mark.parametrize("scales", ["dyadic", "file"])
@pytest.mark.parametrize("model", ["saige_model.npz", "saige_model_quant.npz"])
@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_p1_scan_packed_equals_scan_f64(model, cls, scales):
    """N = 1000, every class, the file's samples as they are and a permuted strict subset of a wider file; 430 rows in
    chunks of 131 (1 MiB of float64 rows): three whole chunks and a tail of 37.  Bit for bit against scan_f64 of the
    host-decoded rows, and against the oracle with assert_table_close.  "dyadic": scales of 2^-6 / 2^-14, every sum of a
    row exact, so the table passes assert_table_close as it stands (AF, mac, num bit-exact).  "file": the scales files
    carry (1/127, 1e-4: products that round, which is where one rounding and two differ); the sums of a row then depend
    on the order of the additions, on the device and in the oracle alike, and AF / mac are held to 1e-9 as
    test_baseline_c3_real_dosages holds sgx_scan_f64's."""
    from oracle import Oracle
    from saigegds_amd._lib import Scanner
    sm = scan_model(model)
    m = 3 * 131 + 37
    codes, _ = P.golden_codes(m)
    _, miss, scale, offset = P.CLASSES[cls]
    exact = scales == "dyadic"
    if exact:
        scale, offset = P.DYADIC[cls]
    raw = P.stored_rows(cls, P.dosages(m, 1000, 31, codes), scale if exact else None, offset)
    assert (np.isnan(P.decode(raw, cls, scale, offset)[1])).all()                   # the all-missing row
    if miss is not None:
        assert (raw == miss).sum() > 1000
    wide, sel = P.widen(raw, 1103, 5)
    orc = Oracle(sm)
    with Scanner(sm, device=0) as sc:
        sc.set_option("pipe_mb", 1)
        _, valid = _check_scan(sc, raw, cls, scale, offset, None, f"{model} {cls} {scales}", orc, sm.quant, exact)
        assert valid.sum() > m // 3
        _check_scan(sc, wide, cls, scale, offset, sel, f"{model} {cls} {scales} subset of 1103", orc, sm.quant, exact)
        sc.set_option("pipe_mb", 0)
        _check_scan(sc, wide[:50], cls, scale, offset, sel, f"{model} {cls} one chunk")


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_p1_rows_that_start_off_the_16_byte_lines(cls):
    """N = 1003 without a selection: a stored row is 1003, 2006 or 4012 bytes, so the rows of a chunk start at every
    residue of 16 the class allows and the float64 rows at both residues of 16."""
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.nullmod import init_nullmod
    n, m = 1003, 150
    mod = synth.synth_null_model(n, "binary", 0.2, n_cov=2, seed=9)
    sm = init_nullmod(mod, np.arange(n), float("nan"), 4.0, 0.1, 0.05, float(mod.var_ratio[0]))
    _, _, scale, offset = P.CLASSES[cls]
    raw = P.stored_rows(cls, P.dosages(m, n, 77))
    with Scanner(sm, device=0) as sc:
        sc.set_option("pipe_mb", 1)
        _, valid = _check_scan(sc, raw, cls, scale, offset, None, f"N=1003 {cls}")
        assert valid.sum() > m // 3


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("cls", ["dPackedReal16U", "dPackedReal8U"])
def test_p2_scan_packed_at_430k(cls):
    """N = 430 000 (the model of BASELINE's C3), a file of 442 345 samples (not a multiple of 8) of which the model keeps
    430 000 in an order of its own; 200 rows = a chunk of 156 (512 MiB of float64 rows) and a tail."""
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.nullmod import init_nullmod
    n, n_file, m, seed = 430_000, 442_345, 200, 20260
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=3, seed=seed)
    sm = init_nullmod(mod, np.arange(n), float("nan"), 10.0, 0.1, 0.05, float(mod.var_ratio[0]))
    _, miss, scale, offset = P.CLASSES[cls]
    wide = P.stored_rows(cls, P.dosages(m, n_file, 43))
    sel = np.random.default_rng(2).permutation(n_file)[:n]
    assert (wide == miss).sum() > m * 1000
    with Scanner(sm, device=0) as sc:
        _, valid = _check_scan(sc, wide, cls, scale, offset, sel, f"N=430000 {cls}")
        tot = sc.stats()
    assert valid.sum() > m // 2 and tot["n_variants"] == m


def test_p3_assoc_100snp_through_the_stored_rows(monkeypatch):
    """seqAssocGLMM_SPA on assoc_100snp.gds's annotation/format/DS (dPackedReal8U): the README's 38 survivors, the table of
    sgx_scan_f64 on dosage_real bit for bit, and 1 byte per value over the link."""
    from saigegds_amd import assoc as assoc_mod
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import GdsFile
    from conftest import load_null_model
    path = os.path.join(GOLDEN, "assoc_100snp.gds")
    g = GdsFile(path)
    ds = g.dosage_real()
    z = np.load(os.path.join(GOLDEN, "assoc_100snp.npz"))
    sid = [str(s) for s in z["sample_id"]]
    assert [str(s) for s in g.sample_id()] == sid
    mod = load_null_model("saige_model.npz")
    sm = scan_model("saige_model.npz", mac=10, sample_ids=sid)
    for bl in (50_000, 30):                      # one block; four blocks, the decoder thread ahead of the scan
        with Scanner(sm, device=0) as sc:        # (a call's rows share a launch: the reference is cut as the driver cuts)
            parts = [sc.scan_f64(ds[a:a + bl]) for a in range(0, 100, bl)]
        ref, ref_valid = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        monkeypatch.setattr(assoc_mod, "BLOCK_SIZE", bl)
        timing = {}
        ans = assoc_mod.seqAssocGLMM_SPA(path, mod, mac=10, dsnode="annotation/format/DS", verbose=False, timing=timing)
        keep = ref_valid.astype(bool)
        assert len(ans["id"]) == 38 == int(keep.sum())
        assert [int(v) for v in ans["id"][:3]] == [4, 12, 14]
        for col, k in (("AF.alt", 0), ("mac", 1), ("beta", 3), ("SE", 4), ("pval", 5), ("p.norm", 6)):
            assert _same(np.asarray(ans[col]), ref[keep][:, k]), col
        assert np.array_equal(ans["num"], ref[keep][:, 2].astype(np.int32)) and np.array_equal(ans["converged"], ref[keep][:, 7] == 1)
        assert timing["decoded_bytes"] == 100 * 1000          # n_variants * n_file_samp, 1 byte per value


def test_p4_dosage_block_from_stored_rows():
    """load_packed == load of the decoded rows: the three arrays, then scan() and burden() bit for bit.  600 rows at
    pipe_mb = 1: the float32 rows (4000 and 4412 bytes) are loaded in three chunks, 262 + 262 + 76 and 237 + 237 + 126,
    the third into the pipeline buffer of the first; the 2-byte classes in two chunks, the 1-byte ones in one."""
    from saigegds_amd._lib import Scanner
    sm = scan_model("saige_model.npz", mac=0.0, maf=0.0, missing=1.0)
    m, per = 600, 10
    assert m > 2 * ((1 << 20) // (4 * 1103))
    codes, _ = P.golden_codes(m)
    x = P.dosages(m, 1000, 12, codes)
    rng = np.random.default_rng(3)
    grp_ptr = np.arange(0, m + 1, per)
    var_idx = rng.permutation(m).astype(np.int32)
    with Scanner(sm, device=0) as sc:
        sc.set_option("pipe_mb", 1)
        for cls in P.CLASSES:
            _, _, scale, offset = P.CLASSES[cls]
            raw = P.stored_rows(cls, x)
            wide, sel = P.widen(raw, 1103, 8)
            dec = P.decode(raw, cls, scale, offset)
            with sc.dosage_block(np.float64, m) as ref_blk:
                nv, sm_, st = ref_blk.load(dec)
                ref, ref_valid = ref_blk.scan()
                flip = (st > nv).astype(np.uint8)
                with np.errstate(invalid="ignore", divide="ignore"):
                    mean = np.where(flip != 0, 2 - st / nv, st / nv)
                w = rng.random((m, 3)) / per
                w[rng.random((m, 3)) < 0.2] = np.nan
                args = (grp_ptr, var_idx, flip[var_idx], w, mean[var_idx, None] * w)
                rb, rb_valid = ref_blk.burden(*args)
            for r, s, what in ((raw, None, cls), (wide, sel, cls + " subset of 1103")):
                with sc.dosage_block(np.float64, m) as blk:
                    nv2, sm2, st2 = blk.load_packed(r, cls, scale, offset, s)
                    assert np.array_equal(nv2, nv) and np.array_equal(st2, st) and _same(sm2, sm_), what
                    out, valid = blk.scan()
                    assert np.array_equal(valid, ref_valid) and _same(out, ref), what
                    ob, vb = blk.burden(*args)
                    assert np.array_equal(vb, rb_valid) and _same(ob, rb), what
            assert ref_valid.sum() > m // 2 and rb_valid.sum() > rb_valid.size // 2


def test_p4_aggregate_drivers_on_a_packed_real_file(tmp_path):
    """seqAssocGLMM_spaBurden / _spaACAT_O on a written file with a dPackedReal16U node (1103 samples, the model's 1000
    among them in another order) equal the same calls on GenotypeSource(dosage = decoded rows) exactly."""
    import aggregate_ds_ref as R
    from saigegds_amd.aggregate import seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaBurden
    from saigegds_amd.assoc import GenotypeSource
    cls = "dPackedReal16U"
    _, _, scale, offset = P.CLASSES[cls]
    mod = R.golden_model()
    m = 96
    codes, _ = P.golden_codes(m)
    raw = P.stored_rows(cls, P.dosages(m, 1000, 21, codes))
    wide, sel = P.widen(raw, 1103, 4)
    sid = [f"x{i}" for i in range(1103)]
    for k, s in enumerate(sel):
        sid[s] = str(mod.sample_id[k])
    path = P.write_ds_file(tmp_path / "ds16.gds", wide, cls, scale, offset, sid)
    units = [np.arange(s, s + 12) + 1 for s in range(0, m, 12)]
    src = GenotypeSource(sid, dosage=P.decode(wide, cls, scale, offset))
    for drv in (seqAssocGLMM_spaBurden, seqAssocGLMM_spaACAT_O):
        for budget in (None, 30 * 8000):                      # one batch; batches of 30 rows
            a = drv(path, mod, units, verbose=False, ds_budget=budget)
            b = drv(src, mod, units, verbose=False, ds_budget=budget)
            R.same_dicts(a, b, f"{drv.__name__} budget {budget}")
            assert np.isfinite(np.asarray(a["pval" if "pval" in a else "pval.b1_1"])).sum() >= len(units) // 2


def test_p5_bad_arguments_leave_the_handle_usable():
    from saigegds_amd import _lib
    from saigegds_amd._lib import Scanner, SgxError
    L = _lib.load()
    sm = scan_model("saige_model.npz")
    codes, _ = P.golden_codes(40)
    cls = "dPackedReal16U"
    _, _, scale, offset = P.CLASSES[cls]
    raw = P.stored_rows(cls, P.dosages(40, 1000, 1, codes))
    wide, sel = P.widen(raw, 1103, 6)
    bad_hi, bad_lo = sel.copy(), sel.copy()
    bad_hi[17], bad_lo[999] = 1103, -1
    with Scanner(sm, device=0) as sc:
        ref, ref_valid = sc.scan_packed(raw, cls, scale, offset)
        out, valid = np.empty((40, 8)), np.zeros(40, dtype=np.uint8)
        nv, sm_, st = np.empty(40, dtype=np.int32), np.empty(40), np.empty(40, dtype=np.int64)
        cases = [
            ("unknown class", lambda: sc.scan_packed(raw, 5, scale, offset)),
            ("unknown class", lambda: sc.scan_packed(raw, -1, scale, offset)),
            ("n_file_samp", lambda: sc.scan_packed(raw[:, :999], cls, scale, offset)),
            ("n_file_samp", lambda: sc.scan_packed(wide[:, :990], cls, scale, offset, np.minimum(sel, 989))),
            ("no selection", lambda: sc.scan_packed(wide, cls, scale, offset)),
            ("outside the file", lambda: sc.scan_packed(wide, cls, scale, offset, bad_hi)),
            ("outside the file", lambda: sc.scan_packed(wide, cls, scale, offset, bad_lo)),
            ("NULL buffer", lambda: _lib.check(L.sgx_scan_packed(sc._h, None, 2, 1000, scale, offset, None, 40,
                                                                 out.ctypes.data, valid.ctypes.data))),
            ("NULL buffer", lambda: _lib.check(L.sgx_scan_packed(sc._h, raw.ctypes.data, 2, 1000, scale, offset, None, 40,
                                                                 None, valid.ctypes.data))),
        ]
        with sc.dosage_block(np.float64, 40) as blk, sc.dosage_block(np.uint8, 40) as blk8:
            cases += [
                ("unknown class", lambda: blk.load_packed(raw, 9, scale, offset)),
                ("n_file_samp", lambda: blk.load_packed(raw[:, :999], cls, scale, offset)),
                ("no selection", lambda: blk.load_packed(wide, cls, scale, offset)),
                ("outside the file", lambda: blk.load_packed(wide, cls, scale, offset, bad_hi)),
                ("float64 block", lambda: blk8.load_packed(raw, cls, scale, offset)),
                ("holds up to", lambda: blk.load_packed(np.concatenate([raw, raw]), cls, scale, offset)),
                ("NULL buffer", lambda: _lib.check(L.sgx_ds_block_load_packed(sc._h, blk._b, None, 2, 1000, scale, offset, None, 40,
                                                                             nv.ctypes.data, sm_.ctypes.data, st.ctypes.data))),
                ("NULL buffer", lambda: _lib.check(L.sgx_ds_block_load_packed(sc._h, blk._b, raw.ctypes.data, 2, 1000, scale, offset,
                                                                             None, 40, None, sm_.ctypes.data, st.ctypes.data))),
            ]
            for msg, call in cases:
                with pytest.raises(SgxError, match=msg) as ei:
                    call()
                assert ei.value.code == -1, msg                 # SGX_EINVAL
            with pytest.raises(SgxError, match="nothing loaded"):
                blk.scan()                                        # a refused load leaves the block empty
            blk.load_packed(wide, cls, scale, offset, sel)
            o2, v2 = blk.scan()
        o1, v1 = sc.scan_packed(wide, cls, scale, offset, sel)    # the handle still scans, and correctly
        o3, v3 = sc.scan_f64(P.decode(raw, cls, scale, offset))
    for o, v in ((o1, v1), (o2, v2), (o3, v3)):
        assert np.array_equal(v, ref_valid) and _same(o, ref)
    assert ref_valid.sum() > 10
