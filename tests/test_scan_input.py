"""``assoc.ScanInput``, the opened input that every driver reads through: its classification of each input form, the
sample selection, and its readers against the source's own rows.  No GPU, no library."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import packed_ds_cases as P

M = 60          # variants of the written and in-memory forms


def _hard_calls():
    codes, sid = P.golden_codes(M)
    return codes, sid


def _form(name, tmp_path):
    """-> (source, kind, the source's 2-bit rows or None, its dosages [variant, sample] or None, has a raw class)"""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import GdsFile, pack_dosage_2bit
    from saigegds_amd.gds_write import GdsWriter
    codes, sid = _hard_calls()
    if name == "mem.packed":
        return GenotypeSource(sid, packed=pack_dosage_2bit(codes)), "packed", pack_dosage_2bit(codes), None, False
    if name in ("mem.uint8", "mem.int32"):
        dt = np.uint8 if name == "mem.uint8" else np.int32
        ds = np.where(codes == 3, 0xFF if dt == np.uint8 else np.iinfo(np.int32).min, codes).astype(dt)
        return GenotypeSource(sid, dosage=ds), "dosage", None, ds, False
    if name == "mem.float64":
        ds = P.dosages(M, 1000, 4, codes=codes)
        return GenotypeSource(sid, dosage=ds), "dosage", None, ds, False
    if name == "file.genotype":
        path = os.path.join(P.GOLDEN, "grm1k_10k_snp.gds")
        return path, "packed", np.load(os.path.join(P.GOLDEN, "grm1k_10k_snp.npz"))["packed"][:, :250], None, False
    if name == "file.golden_ds":           # annotation/format/DS of the reference's file is packed-real
        path = os.path.join(P.GOLDEN, "assoc_100snp.gds")
        return path, "stored", None, GdsFile(path).dosage_real(), True
    if name == "file.dFloat64":
        ds = P.dosages(M, 1000, 4, codes=codes)
        w = GdsWriter(str(tmp_path / "f64.gds"))
        w.put_attr("FileFormat", "SEQ_ARRAY")
        w.add("sample.id", sid, "none")
        w.add("annotation/format/DS/data", ds, "ZIP_RA", cls="dFloat64", dims=ds.shape)
        w.add("annotation/format/DS/@data", np.ones(M, dtype="<i4").tobytes(), "none", cls="dInt32", dims=(M,))
        w.close()
        return str(tmp_path / "f64.gds"), "dosage", None, ds, False
    cls = name.split(".")[1]
    scale, offset = P.DYADIC[cls]
    raw = P.stored_rows(cls, P.dosages(M, 1000, 4, codes=codes), scale, offset)
    path = P.write_ds_file(tmp_path / "ds.gds", raw, cls, scale, offset, sid)
    return path, "stored", None, P.decode(raw, cls, scale, offset), True


FORMS = ["mem.packed", "mem.uint8", "mem.int32", "mem.float64", "file.genotype", "file.golden_ds", "file.dFloat64",
         "file.dPackedReal16U", "file.dFloat32"]


@pytest.mark.parametrize("subset", [False, True], ids=["all", "subset"])
@pytest.mark.parametrize("form", FORMS)
def test_scan_input(form, subset, tmp_path):
    from saigegds_amd.assoc import GenotypeSource, PackedRows, open_scan_input
    from saigegds_amd.gds import GdsFile, pack_dosage_2bit, unpack_dosage_2bit
    src, kind, packed, ds, raw_class = _form(form, tmp_path)
    gsid = [str(s) for s in (src if isinstance(src, GenotypeSource) else GdsFile(src)).sample_id()]
    n_all = len(gsid)
    n_var = (packed if packed is not None else ds).shape[0]
    pick = np.random.default_rng(11).permutation(n_all)[:n_all - 7] if subset else np.arange(n_all)
    mod = SimpleNamespace(sample_id=[gsid[i] for i in pick])
    inp = open_scan_input(src, mod, "", False)

    assert (inp.kind, inp.n_var, inp.n_all, inp.in_mem) == (kind, n_var, n_all, isinstance(src, GenotypeSource))
    assert inp.node == ("$dosage_alt" if kind == "packed" else "annotation/format/DS")
    sel = np.sort(pick)
    assert inp.sel.dtype == np.int64 and np.array_equal(inp.sel, sel) and inp.n_samp == sel.size
    assert inp.ii.dtype == np.int64 and [mod.sample_id[i] for i in inp.ii] == [gsid[i] for i in sel] == inp.sample_id()
    assert inp.all_samples == (not subset)

    idx = np.array([0, 3, 4, n_var - 1])
    if kind == "packed":
        want = lambda rows: pack_dosage_2bit(unpack_dosage_2bit(rows, n_all)[:, sel])        # noqa: E731
        for off, end in ((0, 9), (5, 6), (n_var - 3, n_var)):
            assert np.array_equal(inp.packed_rows(off, end), want(packed[off:end])), (off, end)
        got = inp.packed_rows_at(idx)
        assert got.flags.c_contiguous and np.array_equal(got, want(packed[idx]))
        assert inp.ds_all is None and inp.ds_dtype is None
    else:
        assert inp.ds_dtype == (ds.dtype if inp.in_mem else np.float64)
        got = inp.dosage_reader(False)(idx)
        assert got.dtype == inp.ds_dtype and got.flags.c_contiguous and np.array_equal(got, ds[idx][:, sel], equal_nan=True)
        blk = inp.read_block(2, 7)
        if kind == "stored":
            assert isinstance(blk, PackedRows) and (blk.sel is None) == (not subset)
            blk = P.decode(blk.raw, blk.cls, blk.scale, blk.offset)[:, sel]
            rows = inp.dosage_reader(True)(idx)                                 # the variants picked here, the samples on the device
            assert isinstance(rows, PackedRows) and rows.raw.shape == (idx.size, n_all) and (rows.sel is None) == (not subset)
            assert np.array_equal(P.decode(*rows.args()[:4])[:, sel], ds[idx][:, sel], equal_nan=True)
        assert np.array_equal(blk, ds[2:7][:, sel], equal_nan=True)

    # as stored unless a scanner was injected -- and only a node with a raw class can go as stored
    assert inp.stored_ok(None) == raw_class and not inp.stored_ok(object)


def test_genotype_blocks_follow_the_patched_module_attributes(monkeypatch):
    """read_block looks GENOTYPE_DECODE up when it is called: stored rows for the device, 2-bit rows for the host."""
    from saigegds_amd import assoc
    path, _, packed, _, _ = _form("file.genotype", None)
    gsid = [str(s) for s in assoc.GdsFile(path).sample_id()]
    inp = assoc.open_scan_input(path, SimpleNamespace(sample_id=gsid), "", False)
    monkeypatch.setattr(assoc, "GENOTYPE_DECODE", "device")
    blk = inp.read_block(10, 14)
    assert isinstance(blk, assoc.StoredGenotypes) and (blk.n_file_samp, blk.n_variants, blk.sel) == (1000, 4, None)
    monkeypatch.setattr(assoc, "GENOTYPE_DECODE", "host")
    assert np.array_equal(inp.read_block(10, 14), packed[10:14])


def test_missing_samples_and_matrix_types():
    from saigegds_amd.assoc import GenotypeSource, open_scan_input
    from saigegds_amd.nullmod import ModelError
    codes, sid = _hard_calls()
    f32 = GenotypeSource(sid, dosage=codes.astype(np.float32))
    with pytest.raises(ModelError, match="Some of sample IDs are not available in the GDS file."):
        open_scan_input(f32, SimpleNamespace(sample_id=sid[:5] + ["nobody"]), "", False)
    with pytest.raises(TypeError, match="matrix of uint8, int32 or float64"):
        open_scan_input(f32, SimpleNamespace(sample_id=sid), "", False)
    inp = open_scan_input(f32, SimpleNamespace(sample_id=sid), "", False, any_matrix=True)     # the single-variant driver
    assert inp.kind == "dosage" and inp.read_block(1, 3).dtype == np.float32
    with pytest.raises(TypeError, match="is.character\\(dsnode\\)"):
        open_scan_input(f32, SimpleNamespace(sample_id=sid), 1, False)
