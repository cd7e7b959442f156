"""CPU checks of the explicit-GRM helpers: the numpy stand-in against the long-double product,
``SparseGRM.subset`` and ``load_grm``."""
import os

import numpy as np
import pytest

import grm_dense_ref as D
import kmat_ref as KR
from saigegds_amd import SparseGRM, load_grm, seqFitDenseGRM, seqFitSparseGRM

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GDS = os.path.join(GOLD, "grm1k_10k_snp.gds")
ARGS = dict(maf=0.005, missing_rate=0.01, max_num_snp=2000, seed=200)


def _sparse(n=57, seed=3, big=0):
    i, j, x = KR.family_matrix(n, seed, big)
    return SparseGRM(sample_id=[f"s{k}" for k in range(n)], n=n, n_markers=123, rel_cutoff=0.125, i=i, j=j, x=x)


def test_family_matrix_is_positive_definite():
    for n, big in [(1, 0), (64, 0), (257, 40)]:
        K = KR.Upper(n, *KR.family_matrix(n, 5, big)).to_dense()
        assert np.array_equal(K, K.T) and np.linalg.eigvalsh(K).min() > 0.4


def test_stand_in_matches_long_double_product():
    sp = _sparse(130, 7, 40)
    K = sp.to_dense()
    rng = np.random.default_rng(1)
    B = rng.standard_normal((3, sp.n))
    ref, amp = KR.dense_product_ld(K, B)
    for op in (KR.KmatRef(sp), KR.KmatRef(K)):
        KR.assert_within_bound(op.crossprod_many(B), ref, amp, sp.n)
        assert np.array_equal(op.diag(), np.diag(K))
    r, c, v = KR.full_pattern(sp.n, sp.i, sp.j, sp.x)
    rp, col, val = KR.csr_of(sp.n, r, c, v)
    ref2, amp2, nnz = KR.csr_product_ld(sp.n, rp, col, val, B)
    KR.assert_within_bound(np.stack([sp.matvec(b) for b in B]), ref2, amp2, nnz)
    assert np.max(np.abs(ref2 - ref)) <= 2.0 ** -60 * float(np.max(amp))
    # the solve: (tau0 diag(1/w) + tau1 K) x = b
    w = rng.uniform(0.05, 0.25, sp.n)
    x, it = KR.KmatRef(sp).pcg(w, [0.3, 0.7], B[0], 500, 1e-12)
    assert 0 < it < 500
    np.testing.assert_allclose((0.3 * np.diag(1 / w) + 0.7 * K) @ x, B[0], atol=1e-5)


def test_subset_matches_dense_indexing():
    sp = _sparse(57, 3, 12)
    K = sp.to_dense()
    rng = np.random.default_rng(2)
    for ix in (rng.permutation(57), rng.permutation(57)[:31], np.array([5])):
        ids = [sp.sample_id[k] for k in ix]
        sub = sp.subset(ids)
        assert sub.sample_id == ids and sub.n == len(ids) and sub.rel_cutoff == sp.rel_cutoff
        assert np.array_equal(sub.to_dense(), K[np.ix_(ix, ix)])
        assert (sub.i <= sub.j).all()
        key = sub.i.astype(np.int64) * sub.n + sub.j
        assert (np.diff(key) > 0).all()
    with pytest.raises(ValueError, match="not in the GRM"):
        sp.subset(["s1", "nobody"])
    with pytest.raises(ValueError, match="unique"):
        sp.subset(["s1", "s1"])


@pytest.mark.parametrize("ext", ["npz", "rds"])
def test_load_grm_round_trip(ext, tmp_path):
    ids = [str(s) for s in np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))["sample_id"][:40]]
    fs, fd = str(tmp_path / f"sp.{ext}"), str(tmp_path / f"de.{ext}")
    sp = seqFitSparseGRM(GDS, sample_id=ids, rel_cutoff=0.05, out_fn=fs, verbose=False, operator_factory=D.NumpyGrm, **ARGS)
    did, K = seqFitDenseGRM(GDS, sample_id=ids, out_fn=fd, verbose=False, operator_factory=D.NumpyGrm, **ARGS)
    back = load_grm(fs)
    assert isinstance(back, SparseGRM)
    assert back.sample_id == sp.sample_id and back.n == sp.n and back.rel_cutoff == sp.rel_cutoff
    assert back.i.dtype == np.int32 and np.array_equal(back.i, sp.i) and np.array_equal(back.j, sp.j)
    assert np.array_equal(back.x, sp.x)
    bid, bK = load_grm(fd)
    assert bid == list(did) and bK.dtype == np.float64 and np.array_equal(bK, K)
    with pytest.raises(ValueError, match="Unknown format"):
        load_grm(str(tmp_path / "grm.txt"))
