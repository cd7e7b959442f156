"""seqAssocGLMM_SPA(firth_pval=) on dosage input, on the device: a float64 DS node that holds the golden hard calls
against the hard-call route (sgx_firth_2bit) bit for bit, and a dPackedReal16 node (rows decoded on the device by
load_packed) against the in-memory float64 matrix of its decoded values bit for bit."""
import numpy as np
import pytest

import packed_ds_cases as P
from conftest import load_null_model

pytestmark = pytest.mark.gpu
M = 400
FIRTH = ("beta.firth", "SE.firth", "cvg.firth")


def _write_f64(path, ds, sample_id):
    """A SeqArray-style file without a genotype node whose annotation/format/DS holds float64 rows."""
    from saigegds_amd.gds_write import GdsWriter
    m = ds.shape[0]
    w = GdsWriter(str(path))
    w.put_attr("FileFormat", "SEQ_ARRAY")
    w.add("sample.id", [str(s) for s in sample_id], "none")
    w.add("variant.id", np.arange(1, m + 1), "none")
    w.add("position", np.arange(1, m + 1) * 100, "none")
    w.add("chromosome", ["1"] * m, "none")
    w.add("allele", ["A,C"] * m, "none")
    w.add("annotation/format/DS/data", np.ascontiguousarray(ds, dtype="<f8"), "ZIP_RA", cls="dFloat64", dims=ds.shape)
    w.add("annotation/format/DS/@data", np.ones(m, dtype="<i4").tobytes(), "none", cls="dInt32", dims=(m,))
    w.close()
    return str(path)


def _same_columns(a, b, what):
    assert list(a) == list(b), what
    flagged = ~np.isnan(np.asarray(a["beta.firth"]))
    assert flagged.sum() > 10 and np.asarray(a["cvg.firth"])[flagged].all(), what
    for k in FIRTH:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, k)


def test_float64_node_of_hard_calls_equals_the_hard_call_route(tmp_path):
    from saigegds_amd.assoc import GenotypeSource, seqAssocGLMM_SPA
    from saigegds_amd.gds import pack_dosage_2bit
    codes, sid = P.golden_codes(M)
    codes[::7] = np.array([2, 1, 0, 3], dtype=np.uint8)[codes[::7]]                     # every 7th row alt-major
    mod = load_null_model("saige_model.npz")
    hard = GenotypeSource(sid, packed=pack_dosage_2bit(codes), variant_id=np.arange(1, M + 1), position=np.arange(1, M + 1) * 100)
    want = seqAssocGLMM_SPA(hard, mod, mac=4, verbose=False, firth_pval=0.05)
    path = _write_f64(tmp_path / "ds64.gds", np.where(codes == 3, np.nan, codes.astype(np.float64)), sid)
    got = seqAssocGLMM_SPA(path, mod, mac=4, verbose=False, firth_pval=0.05)
    assert np.array_equal(got["id"], want["id"]) and np.array_equal(got["pval"] <= 0.05, want["pval"] <= 0.05)
    assert (np.asarray(want["AF.alt"])[~np.isnan(want["beta.firth"])] > 0.5).any()
    _same_columns(want, got, "float64 node of hard calls")


def test_packed_node_equals_the_matrix_of_its_decoded_values(tmp_path):
    from saigegds_amd.assoc import GenotypeSource, seqAssocGLMM_SPA
    cls = "dPackedReal16"
    scale, offset = P.DYADIC[cls]
    codes, sid = P.golden_codes(M)
    raw = P.stored_rows(cls, P.dosages(M, 1000, seed=12, codes=codes), scale, offset)
    path = P.write_ds_file(tmp_path / "ds16.gds", raw, cls, scale, offset, sid)
    mem = GenotypeSource(sid, dosage=P.decode(raw, cls, scale, offset), variant_id=np.arange(1, M + 1),
                         position=np.arange(1, M + 1) * 100)
    mod = load_null_model("saige_model.npz")
    got = seqAssocGLMM_SPA(path, mod, mac=4, verbose=False, firth_pval=0.05)
    want = seqAssocGLMM_SPA(mem, mod, mac=4, verbose=False, firth_pval=0.05)
    assert np.array_equal(got["id"], want["id"])
    _same_columns(want, got, "dPackedReal16 node")
