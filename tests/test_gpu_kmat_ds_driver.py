"""``seqAssocGLMM_spaSKAT(grm_mat=)`` and ``seqAssocGLMM_SPA_cond(grm_mat=)`` on dosage input on the device (DESIGN.md
8i): on a float64 and a uint8 in-memory dosage source against the same call with the numpy stand-in blocks of
tests/kmat_ds_ref.py (float64 CG, the device loop's stopping rule), and on a packed-real file written by the build's
own writer against the host-decoded rows.

Bound on Q / pval / pval.cond: kmat_ds_ref.DRIVER_TOL = 10 x the distance of the stand-in's float64 form at
tol = 1e-5 from the long-double Phi^K (tests/test_kmat_ds_ref.py measures it), the project's rule of
tests/cond_kmat_ref.py.  Packed-real input is held to the host-decoded rows bit for bit: the block holds the same
doubles either way.
"""
import numpy as np
import pytest

import kmat_ds_ref as KD
import skat_kmat_ref as M
from test_kmat_ds_ref import family, skat_case

pytestmark = pytest.mark.gpu


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    k = ~np.isnan(a)
    e = float(np.abs(a[k] / b[k] - 1).max()) if k.any() else 0.0
    print(f"{what}: device against the stand-in {e:.3g} (bound {KD.DRIVER_TOL:.3g})")
    assert e <= KD.DRIVER_TOL, what


def hard_u8(n_var=100):
    """uint8 dosages beyond hard calls (a 3 among them, so that the source is not reduced to 2-bit rows)."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:n_var], 1000)
    ds = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    ds[7, 5] = 3
    return GenotypeSource([str(s) for s in g["sample_id"]], dosage=ds)


@pytest.mark.parametrize("kind", ["float64", "uint8"])
def test_skat_driver(kind):
    from saigegds_amd import seqAssocGLMM_spaSKAT
    src, mod, units = skat_case()
    if kind == "uint8":
        src = hard_u8()
    K, blocks = family()
    kw = dict(verbose=False, grm_mat=(src.sample_id(), K))
    want = seqAssocGLMM_spaSKAT(src, mod, units, scanner_factory=KD.kmat_ds_scanner_factory("f64", blocks), **kw)
    got = seqAssocGLMM_spaSKAT(src, mod, units, **kw)
    cut = seqAssocGLMM_spaSKAT(src, mod, units, ds_budget=30 * (8000 if kind == "float64" else 1000), **kw)
    assert list(got) == list(want) == list(cut) and "n.iter" in got
    assert np.array_equal(got["n.var"], want["n.var"]) and got["n.iter"].max() > 0
    for c in ("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25"):
        close(got[c], want[c], f"SKAT {kind} {c}")
        assert np.isfinite(got[c]).all()
    for k in got:                           # batches of 30 resident rows: a unit's results depend on its own rows alone
        assert np.array_equal(np.asarray(got[k]), np.asarray(cut[k]), equal_nan=True), k


@pytest.mark.parametrize("kind", ["float64", "uint8"])
def test_cond_driver(kind):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from test_cond_dosage import fractional_case
    src, mod = fractional_case("binary")
    if kind == "uint8":
        src = hard_u8(200)
    K, blocks = family()
    kw = dict(mac=2, verbose=False, grm_mat=(src.sample_id(), K))
    want = seqAssocGLMM_SPA_cond(src, mod, [30, 77], scanner_factory=KD.kmat_ds_scanner_factory("f64", blocks), **kw)
    got = seqAssocGLMM_SPA_cond(src, mod, [30, 77], **kw)
    assert list(got) == list(want) and list(got)[-1] == "n.iter" and list(got["id"]) == list(want["id"])
    assert got["n.iter"].max() > 0 and np.isfinite(got["pval.cond"]).sum() >= 150
    close(got["pval.cond"], want["pval.cond"], f"cond {kind} pval.cond")


def test_packed_real_file_equals_host_decoded_rows(tmp_path):
    import aggregate_ds_ref as R
    import packed_ds_cases as P
    from saigegds_amd import seqAssocGLMM_SPA_cond, seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    from test_cond_dosage import same_tables
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
    src = GenotypeSource(sid, dosage=P.decode(wide, cls, scale, offset))
    K = M.family_K(1103)[0]
    units = [np.arange(s, s + 12) + 1 for s in range(0, m, 12)]
    kw = dict(verbose=False, grm_mat=(sid, K))
    a, b = seqAssocGLMM_spaSKAT(path, mod, units, **kw), seqAssocGLMM_spaSKAT(src, mod, units, **kw)
    R.same_dicts(a, b, "SKAT on the packed-real file")
    assert "n.iter" in a and np.isfinite(np.asarray(a["pval.b1_25"])).sum() >= len(units) // 2
    stats = src.dosage.shape[0]
    ok = np.isfinite(src.dosage[:, sel])
    s = np.where(ok, src.dosage[:, sel], 0).sum(axis=1)
    lead = [int(v) + 1 for v in np.argsort(-np.minimum(s, 2 * ok.sum(axis=1) - s))[:2]]
    a = seqAssocGLMM_SPA_cond(path, mod, lead, mac=1, **kw)
    b = seqAssocGLMM_SPA_cond(src, mod, lead, mac=1, **kw)
    meta = ("chr", "pos", "rs.id", "ref", "alt")           # the file's own annotation; the in-memory source has defaults
    same_tables({k: v for k, v in a.items() if k not in meta}, {k: v for k, v in b.items() if k not in meta},
                "the conditional scan on the packed-real file")
    assert "n.iter" in a and stats == m and np.isfinite(np.asarray(a["pval.cond"])).sum() >= m // 2
