"""seqFitLDpruning's host logic on the numpy engine of tests/ld_ref.py against the one-candidate-at-a-time rule:
block sizes, chromosome runs, windows that retire in the middle of a block, slide_max_n, sample and variant subsets,
the refusals, the export, and the unchanged default output of write_seqarray_genotypes."""
import hashlib

import numpy as np
import pytest

import ld_cases as LC
import ld_ref as R
from saigegds_amd import GenotypeSource, seqFitLDpruning
from saigegds_amd.gds import GdsFile
from saigegds_amd.gds_write import write_seqarray_genotypes

MAF, MISS = 0.05, 0.05


@pytest.fixture(scope="module")
def data():
    codes, chrom, pos, ids = LC.ld_source(**LC.DRIVER_CPU)
    n = codes.shape[1]
    src = GenotypeSource([f"s{i}" for i in range(n)], packed=R.pack(codes), variant_id=ids, chromosome=chrom, position=pos)
    return dict(codes=codes, chrom=chrom, pos=pos, ids=ids, src=src, n=n)


def _same(got, want):
    assert list(got) == list(want)
    for c in want:
        assert got[c].tolist() == list(want[c]), c


def _run(d, **kw):
    kw.setdefault("maf", MAF)
    kw.setdefault("missing_rate", MISS)
    return seqFitLDpruning(d["src"], verbose=False, engine_factory=R.NumpyLdEngine, **kw)


@pytest.mark.parametrize("block", [1, 7, 256])
@pytest.mark.parametrize("bp,max_n", [(500_000, None), (300, None), (3000, 5)])
def test_driver_equals_sequential_rule(data, block, bp, max_n):
    """Three autosome runs (1, chr7, 2; chrX is skipped) with repeated positions and 2 % missing; at 300 bp window rows
    retire in the middle of a block of 256."""
    d = data
    want = R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, bp, max_n)
    got = _run(d, ld_threshold=0.2, slide_max_bp=bp, slide_max_n=max_n, block=block)
    _same(got, want)
    assert list(want) == ["1", "chr7", "2"]
    n_cand = int(R.marker_ok(d["codes"], MAF, MISS)[[c != "chrX" for c in d["chrom"]]].sum())
    frac = sum(len(v) for v in want.values()) / n_cand
    assert 0.1 < frac < 0.9, frac                                  # there is LD to prune, and not everything goes


def test_window_rows_retire_inside_a_block(data):
    """The case above at 300 bp really has, inside one block of 256, a kept variant that is out of range for a later
    candidate of the same block and run."""
    d = data
    want = R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, 300)
    kept = np.flatnonzero(np.isin(d["ids"], want["1"]))
    assert d["pos"][kept[-1]] - d["pos"][kept[0]] > 300 and kept[-1] < 256


def test_all_chromosomes_and_subsets(data):
    d = data
    want = R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.5, MAF, MISS, 2000, autosome_only=False)
    got = _run(d, ld_threshold=0.5, slide_max_bp=2000, autosome_only=False, block=7)
    _same(got, want)
    assert "chrX" in got
    # a sample subset: rows, counts and filter are those of the subset (given in another order: the file's is used)
    sel = LC.subset("DRIVER_CPU", d["n"])
    want = R.prune_ref(d["codes"][:, sel], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, 500_000)
    got = _run(d, sample_id=[f"s{i}" for i in sel[::-1]], block=7)
    _same(got, want)
    # variant_id restricts the candidates
    cand = d["ids"][::3]
    want = R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, 500_000, candidates=cand)
    got = _run(d, variant_id=cand, block=256)
    _same(got, want)
    assert all(np.isin(v, cand).all() for v in got.values())


def test_one_engine_call_per_block(data):
    d = data
    made = []

    def factory(n, bpv):
        made.append(R.NumpyLdEngine(n, bpv))
        return made[-1]

    seqFitLDpruning(d["src"], verbose=False, engine_factory=factory, maf=MAF, missing_rate=MISS, block=64)
    ok = R.marker_ok(d["codes"], MAF, MISS)
    per_run = [int(ok[[c == name for c in d["chrom"]]].sum()) for name in ("1", "chr7", "2")]
    assert len(made) == 1 and made[0].calls == sum(-(-m // 64) for m in per_run)
    assert made[0].window_len == 0                                 # reset after the last run


def test_window_over_budget_names_slide_max_n(data):
    with pytest.raises(MemoryError, match="slide_max_n"):
        seqFitLDpruning(data["src"], verbose=False, maf=MAF, missing_rate=MISS, block=7,
                        engine_factory=lambda n, b: R.NumpyLdEngine(n, b, max_rows=3))
    got = seqFitLDpruning(data["src"], verbose=False, maf=MAF, missing_rate=MISS, block=7, slide_max_n=3,
                          engine_factory=lambda n, b: R.NumpyLdEngine(n, b, max_rows=3))
    d = data
    _same(got, R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, 500_000, 3))


def test_refusals(data):
    d = data
    pos = d["pos"].copy()
    pos[20] = pos[19] - 1
    bad = GenotypeSource(d["src"].sample_id(), packed=d["src"].packed, variant_id=d["ids"], chromosome=d["chrom"], position=pos)
    with pytest.raises(ValueError, match="positions decrease"):
        seqFitLDpruning(bad, verbose=False, engine_factory=R.NumpyLdEngine)
    ds = GenotypeSource(d["src"].sample_id(), dosage=d["codes"].astype(np.float64).clip(0, 2))
    with pytest.raises(NotImplementedError):
        seqFitLDpruning(ds, verbose=False, engine_factory=R.NumpyLdEngine)
    for kw in (dict(ld_threshold=-0.1), dict(ld_threshold=1.5), dict(ld_threshold=float("nan")), dict(ld_threshold="0.2"),
               dict(maf=0.6), dict(missing_rate=-1.0), dict(slide_max_bp=-1), dict(slide_max_n=0), dict(block=0),
               dict(block=257)):
        with pytest.raises(ValueError):
            _run(d, **kw)
    with pytest.raises(ValueError, match="sample_id"):
        _run(d, sample_id=["nobody"])
    with pytest.raises(ValueError, match="variant_id"):
        _run(d, variant_id=[int(d["ids"][0]), 7])


def test_dosage_only_file_is_refused(tmp_path):
    from saigegds_amd.gds_write import GdsWriter
    fn = str(tmp_path / "ds.gds")
    w = GdsWriter(fn)
    w.put_attr("FileFormat", "SEQ_ARRAY")
    w.add("sample.id", ["a", "b"], "none")
    w.add("variant.id", np.arange(1, 4), "none")
    w.add("position", np.arange(1, 4), "none")
    w.add("chromosome", ["1"] * 3, "none")
    w.add("allele", ["A,C"] * 3, "none")
    w.add("annotation/format/DS/data", np.zeros((3, 2), dtype=np.float32), "none")
    w.close()
    with pytest.raises(NotImplementedError):
        seqFitLDpruning(fn, verbose=False, engine_factory=R.NumpyLdEngine)


def test_file_input_and_export(data, tmp_path):
    """The rows written as a SeqArray file prune to the same ids; save_gdsfn, reopened, holds exactly the kept rows,
    ids, positions and chromosomes; and that file prunes to itself."""
    d = data
    fn, out = str(tmp_path / "in.gds"), str(tmp_path / "pruned.gds")
    write_seqarray_genotypes(fn, d["src"].packed, d["n"], sample_id=d["src"].sample_id(), variant_id=d["ids"],
                             position=d["pos"], chromosome=d["chrom"], allele=["G,T"] * len(d["ids"]))
    want = R.prune_ref(d["codes"], d["chrom"], d["pos"], d["ids"], 0.2, MAF, MISS, 500_000)
    got = seqFitLDpruning(fn, verbose=False, engine_factory=R.NumpyLdEngine, maf=MAF, missing_rate=MISS, block=7,
                          save_gdsfn=out)
    _same(got, want)
    kept = np.flatnonzero(np.isin(d["ids"], np.concatenate([want[c] for c in want])))
    g = GdsFile(out)
    assert np.asarray(g.read("variant.id")).tolist() == d["ids"][kept].tolist()
    assert np.asarray(g.read("position")).tolist() == d["pos"][kept].tolist()
    assert [str(c) for c in g.read("chromosome")] == [d["chrom"][i] for i in kept]
    assert [str(a) for a in g.read("allele")] == ["G,T"] * kept.size
    assert g.sample_id() == d["src"].sample_id()
    packed, n, _ = g.dosage_alt_packed()
    assert n == d["n"] and np.array_equal(R.unpack(packed, n), d["codes"][kept])
    again = seqFitLDpruning(out, verbose=False, engine_factory=R.NumpyLdEngine, maf=MAF, missing_rate=MISS)
    _same(again, want)


def test_writer_defaults_unchanged(tmp_path):
    """write_seqarray_genotypes without the new arguments writes the bytes it wrote before (the digests of the file
    as the previous version of the writer produced it), for whole-byte and odd-sized rows."""
    rng = np.random.default_rng(5)
    for n, m, compress, want in ((12, 9, "none", DIGESTS[0]), (7, 5, "none", DIGESTS[1])):
        fn = str(tmp_path / f"w{n}.gds")
        write_seqarray_genotypes(fn, R.pack(rng.integers(0, 4, (m, n), dtype=np.uint8)), n, compress=compress, chromosome="3")
        assert hashlib.sha256(open(fn, "rb").read()).hexdigest() == want


DIGESTS = ("df79582e47075b2769d72efc85bd780260d5102bb8a2a91a237f6b0e88b6012e",
           "77e3a728b28ae58cbcbf3e4c133e50028a10c028f4a17bd8f824fdbc128bd8ae")
