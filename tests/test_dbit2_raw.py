"""genotype/data rows as stored (GdsFile.genotype_raw_range) and the block rule of the stored route: no GPU."""
import os

import numpy as np
import pytest

import dbit2_cases as D


def _check_range(g, v0, v1, n, sel):
    """the stored bytes, decoded in numpy by the rule, are dosage_alt_packed_range's rows"""
    raw, bit0, n_rows = g.genotype_raw_range(v0, v1)
    m = v1 - v0
    rows = m if n_rows is None else int(np.sum(n_rows))
    assert raw.dtype == np.uint8 and bit0 in (0, 4) and raw.size == (bit0 + rows * n * 4 + 7) // 8
    got = D.decode(raw, bit0, n, n_rows, m, sel)
    ref = g.dosage_alt_packed_range(v0, v1, sel)
    assert got.shape == ref.shape and np.array_equal(got, ref), (v0, v1, n, sel is not None)
    return raw, bit0, n_rows


def test_raw_range_of_the_reference_file():
    from saigegds_amd.gds import GdsFile
    g = GdsFile(os.path.join(D.GOLDEN, "grm1k_10k_snp.gds"))
    m, n = g.genotype_dims()
    assert (m, n) == (10000, 1000) and g.genotype_raw_row_bytes() == 500
    z = np.load(os.path.join(D.GOLDEN, "grm1k_10k_snp.npz"))
    perm = np.random.default_rng(1).permutation(n)
    for v0, v1 in ((0, 300), (4321, 4400), (9999, 10000)):
        raw, bit0, n_rows = _check_range(g, v0, v1, n, None)
        assert bit0 == 0 and n_rows is None and raw.size == (v1 - v0) * 500
        assert np.array_equal(D.decode(raw, bit0, n, None, v1 - v0), z["packed"][v0:v1, :250])
        _check_range(g, v0, v1, n, perm)
    raw, bit0, n_rows = g.genotype_raw_range(10, 10)
    assert raw.size == 0 and n_rows is None


@pytest.mark.parametrize("compress", ["none", "LZMA_RA", "ZIP_RA"])
@pytest.mark.parametrize("n", [37, 1001])
def test_raw_range_of_written_files(tmp_path, n, compress):
    """An odd number of samples: odd rows start on a half byte.  Sites of one row (write_seqarray_genotypes) and files
    with multi-row sites (write_seqarray_alleles), ranges that start mid-file, with and without a permuted selection."""
    from saigegds_amd.gds import GdsFile, pack_dosage_2bit
    from saigegds_amd.gds_write import write_seqarray_genotypes
    m = 41
    al = D.alleles(m, n, 5 + n)
    codes = D.codes_of(al)
    single = al.copy()
    single[D.TWO_ROWS], single[D.THREE_ROWS] = al[0], al[4]
    fn = str(tmp_path / "g.gds")
    write_seqarray_genotypes(fn, pack_dosage_2bit(D.codes_of(single)), n, compress=compress, ra_block=700)
    g = GdsFile(fn)
    assert g.genotype_raw_row_bytes() == (n * 4 + 7) // 8
    rng = np.random.default_rng(n)
    sel = rng.permutation(n)[:n - 5]
    for v0, v1 in ((0, m), (1, m), (7, 8), (12, 31), (m - 1, m)):
        for s in (None, sel):
            raw, bit0, n_rows = _check_range(g, v0, v1, n, s)
            assert n_rows is None and bit0 == (4 if v0 % 2 else 0)          # n is odd: odd rows start on a half byte
    g = GdsFile(D.write_file(tmp_path / "a.gds", al, compress=compress, ra_block=700))
    for v0, v1 in ((0, m), (1, m), (D.TWO_ROWS, D.TWO_ROWS + 1), (D.TWO_ROWS + 1, D.THREE_ROWS + 1), (D.THREE_ROWS + 1, m), (3, 9)):
        for s in (None, sel):
            raw, bit0, n_rows = _check_range(g, v0, v1, n, s)
            multi = v0 <= D.TWO_ROWS < v1 or v0 <= D.THREE_ROWS < v1
            assert (n_rows is not None) == multi
            if multi:
                assert n_rows.dtype == np.int32 and n_rows.size == v1 - v0 and n_rows.max() in (2, 3)
    raw, bit0, n_rows = g.genotype_raw_range(0, m)
    assert n_rows[D.TWO_ROWS] == 2 and n_rows[D.THREE_ROWS] == 3 and int(n_rows.sum()) == m + 3
    # the rule gives the codes the allele indices were written from (digit 3 in one row only is not missing)
    assert np.array_equal(D.decode(raw, bit0, n, n_rows, m), pack_dosage_2bit(codes))
    assert (codes[D.ALL_MISSING] == 3).all() and (codes[D.MONOMORPHIC] == 0).all() and (codes[D.TWO_ROWS] == 3).any()


def test_block_rule_of_the_stored_genotypes(tmp_path, monkeypatch):
    """Blocks of the stored route hold packed_block_size(raw_row_bytes) variants, and what read_block hands on is the
    stored rows (device) or 2-bit rows (host)."""
    from saigegds_amd import assoc
    from saigegds_amd.assoc import BLOCK_SIZE, StoredGenotypes, packed_block_size
    assert assoc.GENOTYPE_DECODE in ("device", "host")
    assert packed_block_size(215_000) == (1 << 30) // 215_000 == 4994       # allele codes at N = 430 000
    assert packed_block_size(500) == BLOCK_SIZE
    al = D.alleles(30, 1001, 3)
    fn = D.write_file(tmp_path / "a.gds", al)
    from saigegds_amd.gds import GdsFile
    g = GdsFile(fn)
    seen = {}

    def fake_scan_blocks(make_scanner, ngpu, blocks, read_block, packed_rows, out, valid, timing=None):
        seen["blocks"] = list(blocks)
        seen["first"] = read_block(*blocks[min(1, len(blocks) - 1)])
        raise RuntimeError("stop here")

    from conftest import load_null_model
    mod = load_null_model("saige_model.npz")
    sid = [str(s) for s in mod.sample_id]
    fn2 = D.write_file(tmp_path / "b.gds", al, sample_id=sid + ["extra"])
    from saigegds_amd import _lib
    real = _lib.load()

    class OneDevice:                                        # (the driver asks for a device before it scans)
        def __getattr__(self, name):
            return getattr(real, name)

        def sgx_device_count(self):
            return 1

    monkeypatch.setattr(_lib, "load", OneDevice)
    monkeypatch.setattr(assoc, "scan_blocks", fake_scan_blocks)
    monkeypatch.setattr(assoc, "PACKED_BLOCK_BYTES", 7 * g.genotype_raw_row_bytes() + 3)
    for mode in ("device", "host"):
        monkeypatch.setattr(assoc, "GENOTYPE_DECODE", mode)
        with pytest.raises(RuntimeError, match="stop here"):
            assoc.seqAssocGLMM_SPA(fn2, mod, verbose=False)
        blk = seen["first"]
        if mode == "device":
            assert seen["blocks"][:2] == [(0, 7), (7, 14)] and seen["blocks"][-1] == (28, 30)
            assert isinstance(blk, StoredGenotypes) and blk.n_file_samp == 1001 and blk.n_variants == 7 and blk.sel is not None
            assert blk.n_rows is not None and blk.n_rows[D.TWO_ROWS - 7] == 2 and blk.bit0 == 4     # row 7 of 1001 samples
            assert blk.nbytes == blk.raw.size == (4 + 8 * 1001 * 4 + 7) // 8
            assert np.array_equal(D.decode(blk.raw, blk.bit0, 1001, blk.n_rows, 7, blk.sel),
                                  g.dosage_alt_packed_range(7, 14, blk.sel))
        else:
            assert seen["blocks"] == [(0, 30)]
            assert isinstance(blk, np.ndarray) and blk.shape == (30, 250)
    monkeypatch.setattr(assoc, "GENOTYPE_DECODE", "gpu")
    with pytest.raises(ValueError, match="GENOTYPE_DECODE"):
        assoc.seqAssocGLMM_SPA(fn2, mod, verbose=False)


def test_a_site_of_more_rows_than_the_device_takes_is_decoded_on_the_host(tmp_path, monkeypatch):
    """sgx_scan_dbit2 takes up to 16 stored rows per variant; a block with a wider site keeps the host decoder."""
    from conftest import load_null_model
    from saigegds_amd import _lib, assoc
    from saigegds_amd.gds import GdsFile
    mod = load_null_model("saige_model.npz")
    al = D.alleles(12, 1000, 8)
    al[5, 0, 0], al[5, 1, 1] = 4 ** 16, 4 ** 16 - 2          # 17 rows
    fn = D.write_file(tmp_path / "w.gds", al, sample_id=[str(s) for s in mod.sample_id])
    g = GdsFile(fn)
    assert g.genotype_raw_range(0, 12)[2][5] == 17 == assoc.MAX_STORED_ROWS + 1
    real = _lib.load()

    class OneDevice:
        def __getattr__(self, name):
            return getattr(real, name)

        def sgx_device_count(self):
            return 1

    got = []

    def fake_scan_blocks(make_scanner, ngpu, blocks, read_block, packed_rows, out, valid, timing=None):
        got.extend(read_block(*b) for b in blocks)
        raise RuntimeError("stop here")

    monkeypatch.setattr(_lib, "load", OneDevice)
    monkeypatch.setattr(assoc, "scan_blocks", fake_scan_blocks)
    monkeypatch.setattr(assoc, "GENOTYPE_DECODE", "device")
    monkeypatch.setattr(assoc, "BLOCK_SIZE", 4)
    with pytest.raises(RuntimeError, match="stop here"):
        assoc.seqAssocGLMM_SPA(fn, mod, verbose=False)
    assert [type(b).__name__ for b in got] == ["StoredGenotypes", "ndarray", "StoredGenotypes"]
    assert np.array_equal(got[1], g.dosage_alt_packed_range(4, 8)) and got[1][1, 0] & 15 == 0b0101
