"""seqFitKING on the device (saigegds_amd/king.py): a SeqArray file of the planted pedigree against the
numpy-engine driver, the vignette's chain LD pruning -> KING -> unrelated set -> PCA -> projection, and the golden file."""
import os

import numpy as np
import pytest

import grm_ref as R
import king_ref as K

pytestmark = pytest.mark.gpu
N, M = 257, 20000


@pytest.fixture(scope="module")
def gds(tmp_path_factory):
    from saigegds_amd.gds_write import write_seqarray_genotypes
    p, _ = K.planted(N, M)
    fn = str(tmp_path_factory.mktemp("king") / "ped.gds")
    sid = [f"s{i}" for i in range(N)]
    write_seqarray_genotypes(fn, R.pack(p.codes), N, sample_id=sid, position=1000 * np.arange(1, M + 1))
    return fn, p, sid


def _same(a, b):
    assert a.sample_id == b.sample_id and a.n == b.n and a.n_markers == b.n_markers and a.kin_cutoff == b.kin_cutoff
    assert np.array_equal(a.i, b.i) and np.array_equal(a.j, b.j) and np.array_equal(a.n_snp, b.n_snp)
    for x, y in ((a.kinship, b.kinship), (a.IBS0, b.IBS0)):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_file_equals_numpy_engine(gds):
    from saigegds_amd import seqFitKING
    fn, p, sid = gds
    got = seqFitKING(fn, verbose=False, **K.FILTER)
    _same(got, seqFitKING(fn, verbose=False, operator_factory=K.NumpyKing, **K.FILTER))
    assert got.n_markers == M
    pairs = [(int(a), int(b)) for a, b in zip(got.i, got.j)]
    assert set(pairs) == set(p.planted)
    assert got.degree().tolist() == [p.planted[pr] for pr in pairs]            # the planted bands
    rng = np.random.default_rng(2)
    sub = [sid[k] for k in rng.permutation(N)[:100]]
    _same(seqFitKING(fn, sample_id=sub, verbose=False, **K.FILTER),
          seqFitKING(fn, sample_id=sub, verbose=False, operator_factory=K.NumpyKing, **K.FILTER))
    sub = sub[:40]
    _same(seqFitKING(fn, sample_id=sub, kin_cutoff=None, verbose=False, **K.FILTER),
          seqFitKING(fn, sample_id=sub, kin_cutoff=None, verbose=False, operator_factory=K.NumpyKing, **K.FILTER))


def test_chain_prune_king_unrelated_pca_project(gds):
    from saigegds_amd import pca_project, seqFitKING, seqFitLDpruning, seqFitPCA, unrelated_set
    fn, p, sid = gds
    kept = np.concatenate(list(seqFitLDpruning(fn, ld_threshold=0.2, maf=0.05, missing_rate=0.05, verbose=False).values()))
    assert 1000 < kept.size <= M
    king = seqFitKING(fn, variant_id=kept, verbose=False, **K.FILTER)
    assert king.n_markers == kept.size
    unrel, rel = unrelated_set(king)
    assert rel and len(unrel) + len(rel) == N
    pos = {s: k for k, s in enumerate(sid)}
    assert not any((min(pos[a], pos[b]), max(pos[a], pos[b])) in p.planted for a in unrel for b in unrel)
    pca = seqFitPCA(fn, sample_id=unrel, variant_id=kept, n_pc=1, snp_loading=True, verbose=False, **K.FILTER)
    pc1 = pca["eigenvect"][:, 0]
    upop = p.pop[[pos[s] for s in unrel]]
    mid = (pc1[upop == 0].mean() + pc1[upop == 1].mean()) / 2
    side = np.sign(pc1[upop == 1].mean() - mid)
    assert ((np.sign(pc1 - mid) == side) == (upop == 1)).all()                 # PC 1 is the population axis
    ids, scores = pca_project(pca, fn, sample_id=rel, verbose=False)
    rpop = p.pop[[pos[s] for s in ids]]
    assert set(rpop.tolist()) == {0, 1}
    assert ((np.sign(scores[:, 0] - mid) == side) == (rpop == 1)).all()        # every relative on its population's side


def test_golden_file():
    from saigegds_amd import seqFitKING
    fn = os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.gds")
    got = seqFitKING(fn, max_num_snp=3000, kin_cutoff=0.0, verbose=False)
    want = seqFitKING(fn, max_num_snp=3000, kin_cutoff=0.0, verbose=False, operator_factory=K.NumpyKing)
    assert got.n == 1000 and 0 < got.n_markers <= 3000 and got.i.size > 0
    _same(got, want)
