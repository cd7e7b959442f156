"""Packed-real dosage nodes as stored (GdsFile.dosage_raw_range) and the block rule of the stored-rows route: no GPU."""
import os

import numpy as np
import pytest

import packed_ds_cases as P

DS = "annotation/format/DS"


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("compress", ["ZIP_RA", "none"])
@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_raw_range_decodes_to_real_range(tmp_path, cls, compress):
    from saigegds_amd.gds import GdsFile
    dt, miss, scale, offset = P.CLASSES[cls]
    m, n = 37, 53
    raw = P.stored_rows(cls, P.dosages(m, n, 7))
    if miss is not None:
        raw[5, 5] = miss
        assert (raw == miss).any() and (raw[1] == miss).all()
    path = P.write_ds_file(tmp_path / "ds.gds", raw, cls, scale, offset, [f"s{i}" for i in range(n)], compress, ra_block=512)
    g = GdsFile(path)
    assert g.dosage_raw_class(DS) == cls and g.dosage_raw_row_bytes(DS) == n * dt.itemsize
    for v0, v1 in ((0, m), (3, 4), (11, 30), (m - 1, m)):
        got, c, sc, of = g.dosage_raw_range(DS, v0, v1)
        assert c == cls and got.dtype == dt and got.shape == (v1 - v0, n)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(raw[v0:v1]).view(np.uint8))      # nothing decoded
        if cls != "dFloat32":
            assert (sc, of) == (scale, offset)
        ref = g.dosage_real_range(DS, v0, v1)
        assert np.isnan(ref).any() or v1 - v0 == 1
        assert _same_bits(P.decode(got, c, sc, of), ref), (cls, v0, v1)


def test_raw_range_of_the_reference_file():
    from saigegds_amd.gds import GdsFile
    g = GdsFile(os.path.join(P.GOLDEN, "assoc_100snp.gds"))
    assert g.dosage_raw_class(DS) == "dPackedReal8U"
    raw, cls, scale, offset = g.dosage_raw_range(DS, 0, 100)
    assert raw.dtype == np.uint8 and raw.shape == (100, 1000) and g.dosage_raw_row_bytes(DS) == 1000
    assert _same_bits(P.decode(raw, cls, scale, offset), g.dosage_real_range(DS, 0, 100))
    assert _same_bits(P.decode(raw[10:37], cls, scale, offset), g.dosage_real()[10:37])
    part = g.dosage_raw_range(DS, 10, 37)[0]
    assert np.array_equal(part, raw[10:37])


def test_raw_range_checks_the_node(tmp_path):
    from saigegds_amd.gds import GdsError, GdsFile
    from saigegds_amd.gds_write import GdsWriter
    w = GdsWriter(str(tmp_path / "f64.gds"))
    x = np.arange(12, dtype="<f8").reshape(3, 4)
    w.add(DS + "/data", x, "none", cls="dFloat64", dims=x.shape)
    raw = np.arange(12, dtype=np.uint8).reshape(3, 4)
    w.add("annotation/format/D2/data", raw, "none", cls="dPackedReal8U", dims=raw.shape, scale=0.01, offset=0.0)
    w.add("annotation/format/D2/@data", np.array([1, 2, 1], dtype="<i4").tobytes(), "none", cls="dInt32", dims=(3,))
    w.close()
    g = GdsFile(str(tmp_path / "f64.gds"))
    assert g.dosage_raw_class(DS) is None                          # dFloat64 keeps the decoded route
    with pytest.raises(GdsError, match="not a packed-real"):
        g.dosage_raw_range(DS, 0, 3)
    with pytest.raises(GdsError, match="more than one value per variant"):      # the @data check of dosage_real_range
        g.dosage_raw_range("annotation/format/D2", 0, 3)


def test_block_rule_of_the_stored_rows_route():
    """min(BLOCK_SIZE, max(1, 1 GiB // raw_row_bytes)) variants per block."""
    from saigegds_amd.assoc import BLOCK_SIZE, packed_block_size
    assert BLOCK_SIZE == 50_000
    assert packed_block_size(1000) == 50_000                        # small rows: .bl_size as everywhere
    assert packed_block_size((1 << 30) // 50_000) == 50_000 and packed_block_size((1 << 30) // 50_000 + 1) == 49_999
    assert packed_block_size(430_000 * 2) == (1 << 30) // 860_000 == 1248      # 16-bit rows at N = 430 000
    assert packed_block_size(430_000) == 2497
    assert packed_block_size(1 << 30) == 1 and packed_block_size((1 << 30) + 1) == 1 and packed_block_size(1 << 40) == 1
    for rb in (1, 999, 21_475, 860_000, 5 << 30):
        assert packed_block_size(rb) == min(BLOCK_SIZE, max(1, (1 << 30) // rb))
        assert packed_block_size(rb) * rb <= max(1 << 30, rb)       # a block never holds more than a GiB (or one row)
