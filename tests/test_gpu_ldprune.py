"""seqFitLDpruning on the device engine against the sequential rule of tests/ld_ref.py: N = 500, M = 3000 of the
synthetic source, from memory and from a file, at two block sizes, and on a second handle."""
import numpy as np
import pytest

import ld_cases as LC
import ld_ref as R

pytestmark = pytest.mark.gpu
MAF, MISS, BP = 0.05, 0.05, 20_000


@pytest.fixture(scope="module")
def data():
    codes, chrom, pos, ids = LC.ld_source(**LC.DRIVER_GPU)
    want = R.prune_ref(codes, chrom, pos, ids, 0.2, MAF, MISS, BP)
    return dict(codes=codes, chrom=chrom, pos=pos, ids=ids, want=want, n=codes.shape[1])


def _same(got, want):
    assert list(got) == list(want)
    for c in want:
        assert got[c].tolist() == list(want[c]), c


def test_driver_on_device_equals_rule(data, tmp_path):
    from saigegds_amd import GenotypeSource, seqFitLDpruning
    from saigegds_amd.gds_write import write_seqarray_genotypes
    d = data
    sid = [f"s{i}" for i in range(d["n"])]
    src = GenotypeSource(sid, packed=R.pack(d["codes"]), variant_id=d["ids"], chromosome=d["chrom"], position=d["pos"])
    kw = dict(ld_threshold=0.2, maf=MAF, missing_rate=MISS, slide_max_bp=BP, verbose=False)
    got = seqFitLDpruning(src, **kw)
    _same(got, d["want"])
    n_kept = sum(len(v) for v in got.values())
    assert 0.1 < n_kept / R.marker_ok(d["codes"], MAF, MISS).sum() < 0.9
    _same(seqFitLDpruning(src, block=64, **kw), d["want"])
    fn = str(tmp_path / "g.gds")
    write_seqarray_genotypes(fn, src.packed, d["n"], sample_id=sid, variant_id=d["ids"], position=d["pos"],
                             chromosome=d["chrom"])
    _same(seqFitLDpruning(fn, **kw), d["want"])
    # bounded by slide_max_n as well, on a sample subset
    sel = LC.subset("DRIVER_GPU", d["n"])
    want = R.prune_ref(d["codes"][:, sel], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, BP, 5)
    _same(seqFitLDpruning(fn, sample_id=[sid[i] for i in sel], slide_max_n=5, **kw), want)


def test_second_handle_same_bits():
    from saigegds_amd._lib import LdEngine
    c = LC.random_codes(4097, 65, 31)
    p = R.pack(c)
    with LdEngine(4097, p.shape[1]) as e1, LdEngine(4097, p.shape[1]) as e2:
        a, b = e1.counts(p, p), e2.counts(p, p)
        f1, f2 = e1.block(p, 0.04), e2.block(p, 0.04)
    assert np.array_equal(a, b) and np.array_equal(a, R.counts(c, c))
    assert np.array_equal(np.tril(f1, -1), np.tril(f2, -1))
