"""The dosage route of ``seqAssocGLMM_SPA_cond`` on the host: the driver with the numpy stand-in scanner of
tests/cond_ds_ref.py (scan: the CPU oracle; cond_set / cond: the dense algebra in double) against the hard-call route,
on fractional dosages, from a file that holds only annotation/format/DS, across batch cuts, and its errors."""
import os

import numpy as np
import pytest

from cond_ds_ref import NumpyCondDsScanner
from test_cond import driver_case, ref_cond_scanner_factory

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def as_dosage(src, dtype, scale=1.0):
    """The hard calls of ``driver_case`` as an in-memory source of dosages: codes * scale, missing 0xFF / NaN."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    codes = unpack_dosage_2bit(src.packed, 1000)
    if dtype == np.uint8:
        ds = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    else:
        ds = np.where(codes == 3, np.nan, codes * scale)
    return GenotypeSource(src.sample_id(), dosage=ds)


def same_tables(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{what}: column {k}"


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_dosage_route_equals_hard_call_route(trait, dtype):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    src, mod = driver_case(trait)
    hard = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=4, verbose=False, scanner_factory=ref_cond_scanner_factory())
    got = seqAssocGLMM_SPA_cond(as_dosage(src, dtype), mod, [30, 77], mac=4, verbose=False, scanner_factory=NumpyCondDsScanner)
    assert list(got.keys()) == list(hard.keys())
    for c in ("id", "chr", "pos", "ref", "alt", "num") + (("converged",) if trait == "binary" else ()):
        assert np.array_equal(np.asarray(got[c]), np.asarray(hard[c])), c
    for c in ("beta.cond", "SE.cond", "pval.cond"):
        assert np.array_equal(np.isnan(got[c]), np.isnan(hard[c])), c
    f = np.isfinite(hard["pval.cond"])
    assert f.sum() >= 150
    e_b = np.abs(got["beta.cond"][f] - hard["beta.cond"][f]) / (1e-9 * np.abs(hard["beta.cond"][f]) + 1e-11 * hard["SE.cond"][f])
    e_s = np.abs(got["SE.cond"][f] - hard["SE.cond"][f]) / (1e-9 * hard["SE.cond"][f])
    e_p = np.abs(got["pval.cond"][f] - hard["pval.cond"][f]) / (1e-8 * hard["pval.cond"][f])
    print(trait, np.dtype(dtype), "beta.cond / SE.cond / pval.cond off by", e_b.max(), e_s.max(), e_p.max(), "x tolerance")
    assert e_b.max() <= 1 and e_s.max() <= 1 and e_p.max() <= 1


def fractional_case(trait="binary"):
    """codes * 0.5 of the 200 golden variants (NaN where missing), the alt-major twins 2 - x of the first 20, a
    monomorphic row and one without a dosage."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import unpack_dosage_2bit
    src, mod = driver_case(trait)
    codes = unpack_dosage_2bit(src.packed, 1000)[:200]
    x = np.where(codes == 3, np.nan, codes * 0.5)
    extra = np.zeros((2, 1000))
    extra[1] = np.nan
    return GenotypeSource(src.sample_id(), dosage=np.concatenate([x, 2 - x[:20], extra])), mod


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_fractional_dosages(trait):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    src, mod = fractional_case(trait)
    ans = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=2, verbose=False, scanner_factory=NumpyCondDsScanner)
    ids = list(ans["id"])
    assert 221 not in ids and 222 not in ids and 30 in ids and 77 in ids
    for c in ("beta.cond", "SE.cond", "pval.cond"):
        a = ans[c]
        assert np.isnan(a[ids.index(30)]) and np.isnan(a[ids.index(77)])           # a conditioning variant itself
        assert np.isfinite(np.delete(a, [ids.index(30), ids.index(77)])).all()
    assert np.all(ans["pval.cond"][np.isfinite(ans["pval.cond"])] > 0)
    n_twin = 0
    for v in range(1, 21):                     # the alt-major twin of a variant: the same test, beta.cond of the other allele
        if v in ids and 200 + v in ids:
            a, b = ids.index(v), ids.index(200 + v)
            n_twin += 1
            assert (ans["AF.alt"][a] > 0.5) != (ans["AF.alt"][b] > 0.5)
            assert abs(ans["beta.cond"][a] + ans["beta.cond"][b]) <= 1e-9 * abs(ans["beta.cond"][a]) + 1e-11 * ans["SE.cond"][a]
            assert abs(ans["SE.cond"][a] - ans["SE.cond"][b]) <= 1e-9 * ans["SE.cond"][a]
            assert abs(ans["pval.cond"][a] - ans["pval.cond"][b]) <= 1e-8 * ans["pval.cond"][a]
            assert np.sign(ans["beta"][a]) == -np.sign(ans["beta"][b])
    assert n_twin >= 5


def file_case():
    """assoc_100snp.gds (only annotation/format/DS) -> path, the same data as an in-memory float64 source, the model."""
    from aggregate_ds_ref import golden_model
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import GdsFile
    path = os.path.join(GOLD, "assoc_100snp.gds")
    f = GdsFile(path)
    ref, alt = f.alleles()
    rs = list(f.read("annotation/id")) if f.node("annotation/id", silent=True) is not None else None
    mem = GenotypeSource(f.sample_id(), dosage=f.dosage_real(), variant_id=np.asarray(f.read("variant.id")),
                         chromosome=list(f.read("chromosome")), position=f.read("position"), rs_id=rs, ref=list(ref), alt=list(alt))
    return path, mem, golden_model()


def test_file_route_equals_in_memory_route():
    from saigegds_amd import seqAssocGLMM_SPA_cond
    path, mem, mod = file_case()
    cond = [mem.variant_id[25], mem.variant_id[63]]            # the two variants of the largest mac (996, 869)
    want = seqAssocGLMM_SPA_cond(mem, mod, cond, mac=1, verbose=False, scanner_factory=NumpyCondDsScanner)
    assert len(want["id"]) >= 50 and np.isfinite(want["pval.cond"]).sum() >= len(want["id"]) - 6
    for dsnode in ("", "annotation/format/DS"):
        got = seqAssocGLMM_SPA_cond(path, mod, cond, mac=1, verbose=False, scanner_factory=NumpyCondDsScanner, dsnode=dsnode)
        same_tables(got, want, f"dsnode={dsnode!r}")


def test_batch_cut(monkeypatch):
    from saigegds_amd import aggregate, seqAssocGLMM_SPA_cond
    src, mod = fractional_case()
    one = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=2, verbose=False, scanner_factory=NumpyCondDsScanner)
    assert NumpyCondDsScanner.last.uploads == 2                 # the set's block, then all rows at once
    monkeypatch.setattr(aggregate, "DS_BUDGET", 60 * 1000 * 8)  # 60 float64 rows a batch: 222 rows in 4 batches
    cut = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=2, verbose=False, scanner_factory=NumpyCondDsScanner)
    assert NumpyCondDsScanner.last.uploads == 1 + 4
    same_tables(cut, one, "4 batches")


def test_bad_conditioning_variants_and_refusals():
    from saigegds_amd import seqAssocGLMM_SPA_cond
    src, mod = fractional_case()
    run = lambda cond, **kw: seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, scanner_factory=NumpyCondDsScanner, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="variant 221 has no valid genotype or is monomorphic"):       # monomorphic
        run([5, 221])
    with pytest.raises(ValueError, match="variant 222 has no valid genotype or is monomorphic"):       # all missing
        run([222])
    for bad in ([], list(range(1, 18)), [5, 9, 5], [5, 100000]):
        with pytest.raises(ValueError, match="condition"):
            run(bad)
    # a scanner whose block has no cond: refused before a row is read, the scanner closed
    from skat_ds_ref import NumpySkatDsScanner

    class Fac(NumpySkatDsScanner):
        closed = 0

        def close(self):
            Fac.closed += 1
            super().close()
    with pytest.raises(NotImplementedError, match="Conditional analysis on dosage input is not implemented."):
        seqAssocGLMM_SPA_cond(src, mod, [5], verbose=False, scanner_factory=Fac)
    assert Fac.closed >= 1 and Fac.last.uploads == 0
