"""CPU: the reference of KING-robust kinship (tests/king_ref.py) on hand-computed cases and on the planted pedigrees
the GPU tests use, ``unrelated_set``, and the host logic of seqFitKING on the numpy stand-in operator."""
import numpy as np
import pytest

import grm_dense_ref as D
import grm_ref as R
import king_ref as K

import saigegds_amd
from saigegds_amd import KingResult, SparseGRM, load_king, seqFitKING, unrelated_set
from saigegds_amd._lib import king_values
from saigegds_amd.king import degree_of


def test_exported_names():
    for name in ("seqFitKING", "KingResult", "load_king", "unrelated_set"):
        assert hasattr(saigegds_amd, name)
    from saigegds_amd._lib import ABI, GrmOperator, SgxGrmKingStats
    assert "sgx_grm_king_counts" in ABI and "sgx_grm_king_pairs" in ABI
    assert hasattr(GrmOperator, "king_counts") and hasattr(GrmOperator, "king_pairs")
    assert [f[0] for f in SgxGrmKingStats._fields_] == ["tiles", "pairs", "ms_kernel", "ms_sort"]


def test_hand_computed_pair():
    x, y = (0, 1, 2, 1, 3), (2, 1, 0, 1, 1)
    c = K.counts(np.array([x, y], dtype=np.uint8).T)
    # markers called in both: 0 .. 3.  x is 1 at markers 1, 3 (y called there); y is 1 at 1, 3 and at 4, where x is
    # missing; both 1 at 1, 3; (0, 2) at marker 0 and (2, 0) at marker 2
    assert c[:, 0, 1].tolist() == [4, 2, 2, 2, 2]
    assert c[:, 1, 0].tolist() == [4, 2, 2, 2, 2]
    assert c[:, 0, 0].tolist() == [4, 2, 2, 2, 0] and c[:, 1, 1].tolist() == [5, 3, 3, 3, 0]
    kin, ibs = K.values(c)
    # D = (2 + 2 - 4) + 4 * 2 = 8, mn = 2: 0.5 - 8 / 8
    assert kin[0, 1] == -0.5 and ibs[0, 1] == 0.5
    assert kin[0, 0] == 0.5 and kin[1, 1] == 0.5 and ibs[0, 0] == 0.0


def test_hand_computed_asymmetric_pair():
    x, y = (1, 1, 1, 0, 2, 3, 0), (1, 0, 3, 0, 0, 1, 2)
    c = K.counts(np.array([x, y], dtype=np.uint8).T)
    # both called: markers 0, 1, 3, 4, 6.  hi: x == 1 at 0, 1 (2 is missing in y).  hj: y == 1 at 0.  hh: 0.
    # ibs0: (2, 0) at 4, (0, 2) at 6
    assert c[:, 0, 1].tolist() == [5, 2, 1, 1, 2]
    assert c[:, 1, 0].tolist() == [5, 1, 2, 1, 2]
    kin, ibs = K.values(c)
    # D = (2 + 1 - 2) + 8 = 9, mn = 1
    assert kin[0, 1] == 0.5 - 9 / 4 and kin[1, 0] == kin[0, 1] and ibs[0, 1] == 2 / 5


def test_no_heterozygote_and_all_missing():
    codes = np.array([[0, 2, 3, 1], [2, 2, 3, 1], [0, 0, 3, 0], [2, 0, 3, 1]], dtype=np.uint8)   # [m = 4, n = 4]
    c = K.counts(codes)
    kin, ibs = K.values(c)
    assert np.isnan(kin[0, 1]) and np.isnan(kin[0, 3]) and np.isnan(kin[0, 0])    # samples 0 and 1: no heterozygote
    assert np.isnan(kin[2]).all() and np.isnan(ibs[2]).all() and (c[:, 2] == 0).all()   # sample 2: all missing
    assert ibs[0, 1] == 0.5 and kin[3, 3] == 0.5
    i, j = K.pairs(c, -1e300)[:2]
    assert i.size == 0                                     # NaN never passes, whatever the cutoff


def test_float_products_equal_integer_products():
    rng = np.random.default_rng(4)
    codes = rng.integers(0, 4, (700, 37), dtype=np.uint8)
    assert np.array_equal(K.counts(codes), K.counts_int(codes))
    assert np.array_equal(K.unpack(R.pack(codes), 37), codes)


def test_library_expression_is_the_reference_expression():
    rng = np.random.default_rng(6)
    c = K.counts(rng.integers(0, 4, (300, 50), dtype=np.uint8))
    a, b = king_values(c), K.values(c)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("n,m", sorted(K.PEDIGREES))
def test_planted_pedigrees_sit_in_their_bands(n, m):
    p, cnt = K.planted(n, m)
    kin, _ = K.values(cnt)
    i, j = np.triu_indices(n, 1)
    want = np.full((n, n), -1, dtype=np.int64)
    for (a, b), d in p.planted.items():
        want[a, b] = d
    assert sorted(set(p.planted.values())) == [0, 1, 2, 3]
    assert not np.isnan(kin[i, j]).any()
    assert np.array_equal(K.band(kin)[i, j], want[i, j])
    # no value within MARGIN of a band edge: the GPU case can never sit on a threshold
    assert np.abs(kin[i, j][:, None] - np.array(K.EDGES)[None, :]).min() >= K.MARGIN
    assert np.array_equal(degree_of(kin[i, j]), want[i, j])


def test_structure_inflates_the_grm_not_king():
    """The reason the feature exists: unrelated pairs of different populations have negative KING kinship, unrelated
    pairs within a population stay below the cutoff -- while the standardised GRM puts those above 0.02."""
    n, m = 257, 20000
    p, cnt = K.planted(n, m)
    kin, _ = K.values(cnt)
    i, j = np.triu_indices(n, 1)
    fam = np.zeros(n, dtype=bool)
    fam[[s for pr in p.planted for s in pr]] = True
    free = ~fam[i] & ~fam[j]
    cross, within = free & (p.pop[i] != p.pop[j]), free & (p.pop[i] == p.pop[j])
    assert cross.sum() > 1000 and within.sum() > 1000
    assert (kin[i, j][cross] < 0).all()
    assert (kin[i, j][within] < K.CUT - K.MARGIN).all()
    G = D.double_gram(p.codes)
    assert (G[i, j][within] > 0.02).all()
    assert (G[i, j][cross] < 0).all()


# ---- unrelated_set
def _king(n, pairs):
    pairs = sorted(pairs)
    i = np.array([a for a, _, _ in pairs], dtype=np.int32)
    j = np.array([b for _, b, _ in pairs], dtype=np.int32)
    k = np.array([x for _, _, x in pairs], dtype=np.float64)
    return KingResult(sample_id=[f"s{q}" for q in range(n)], n=n, n_markers=0, kin_cutoff=0.0, i=i, j=j, kinship=k,
                      IBS0=np.zeros(k.size), n_snp=np.zeros(k.size, dtype=np.int32))


def _idx(ids):
    return [int(s[1:]) for s in ids]


def _check_independent_and_maximal(n, pairs, keep, drop):
    assert sorted(keep + drop) == list(range(n)) and keep == sorted(keep) and drop == sorted(drop)
    rel = {(a, b) for a, b, _ in pairs} | {(b, a) for a, b, _ in pairs}
    assert not any((a, b) in rel for a in keep for b in keep)
    assert all(any((d, a) in rel for a in keep) for d in drop)


def test_unrelated_trio_star_and_empty():
    keep, drop = unrelated_set(_king(5, [(1, 3, 0.25), (2, 3, 0.25)]))      # parents 1, 2 and their child 3
    assert _idx(keep) == [0, 1, 2, 4] and _idx(drop) == [3]
    keep, drop = unrelated_set(_king(6, [(0, 2, 0.1), (1, 2, 0.1), (2, 4, 0.1), (2, 5, 0.1)]))   # a star around 2
    assert _idx(keep) == [0, 1, 3, 4, 5] and _idx(drop) == [2]
    keep, drop = unrelated_set(_king(4, []))
    assert _idx(keep) == [0, 1, 2, 3] and drop == []


def test_unrelated_ties():
    # one relative each: the higher index goes, the earlier sample survives
    keep, _ = unrelated_set(_king(4, [(0, 1, 0.2), (2, 3, 0.2)]))
    assert _idx(keep) == [0, 2]
    # a path 0 - 1 - 2 - 3: 1 and 2 have two relatives each; 1's kinship sum is larger, so 1 goes first, then 3
    keep, _ = unrelated_set(_king(4, [(0, 1, 0.3), (1, 2, 0.1), (2, 3, 0.1)]))
    assert _idx(keep) == [0, 2]
    # the same path with equal sums: the higher index (2) goes first, then 1 (one relative, as 0, but the higher index)
    keep, _ = unrelated_set(_king(4, [(0, 1, 0.1), (1, 2, 0.1), (2, 3, 0.1)]))
    assert _idx(keep) == [0, 3]


def test_unrelated_readmits_for_maximality():
    # a triangle 0 - 1 - 2 with a tail 2 - 3: 2 goes (three relatives), then 1; nothing to re-admit, 3 stays
    pairs = [(0, 1, 0.1), (0, 2, 0.1), (1, 2, 0.1), (2, 3, 0.1)]
    keep, drop = unrelated_set(_king(4, pairs))
    assert _idx(keep) == [0, 3] and _idx(drop) == [1, 2]
    rng = np.random.default_rng(8)
    for n, e in ((30, 25), (60, 120), (40, 300)):
        a, b = rng.integers(0, n, e), rng.integers(0, n, e)
        pairs = sorted({(int(min(x, y)), int(max(x, y))) for x, y in zip(a, b) if x != y})
        pairs = [(x, y, float(rng.uniform(0.05, 0.5))) for x, y in pairs]
        keep, drop = unrelated_set(_king(n, pairs))
        _check_independent_and_maximal(n, pairs, _idx(keep), _idx(drop))
        assert unrelated_set(_king(n, pairs)) == (keep, drop)              # deterministic


def test_unrelated_cutoff_subset_and_sparse_grm():
    pairs = [(0, 1, 0.3), (1, 2, 0.06), (3, 4, 0.2), (4, 5, 0.2), (4, 6, 0.09)]
    kr = _king(8, pairs)
    assert _idx(unrelated_set(kr)[1]) == [1, 4]
    assert _idx(unrelated_set(kr, kin_cutoff=0.1)[1]) == [1, 4]
    assert _idx(unrelated_set(kr, kin_cutoff=0.25)[1]) == [1]
    keep, drop = unrelated_set(kr, sample_id=["s6", "s4", "s1", "s2"])
    assert _idx(keep) == [1, 4] and _idx(drop) == [2, 6]     # (pairs with samples outside the subset are ignored)
    with pytest.raises(ValueError, match="not among"):
        unrelated_set(kr, sample_id=["nobody"])
    # a SparseGRM of the same pairs (plus its diagonal) gives the same set
    i = np.array([a for a, _, _ in pairs] + list(range(8)), dtype=np.int32)
    j = np.array([b for _, b, _ in pairs] + list(range(8)), dtype=np.int32)
    x = np.array([v for _, _, v in pairs] + [1.0] * 8)
    o = np.lexsort((j, i))
    sg = SparseGRM(sample_id=kr.sample_id, n=8, n_markers=0, rel_cutoff=0.05, i=i[o], j=j[o], x=x[o])
    assert unrelated_set(sg) == unrelated_set(kr)
    assert unrelated_set(sg, kin_cutoff=0.25) == unrelated_set(kr, kin_cutoff=0.25)
    with pytest.raises(ValueError, match="KingResult or a SparseGRM"):
        unrelated_set([(0, 1)])


# ---- the driver on the numpy engine
N, M = 60, 3000


@pytest.fixture(scope="module")
def codes():
    return K.pedigree(N, M, 2).codes


def _fit(codes, **kw):
    args = dict(verbose=False, operator_factory=K.NumpyKing, **K.FILTER)
    args.update(kw)
    return seqFitKING(K.source(codes), **args)


def test_driver_pairs_are_the_reference_pairs(codes):
    res = _fit(codes)
    cnt = K.counts(codes)
    i, j, kin, ibs, c5 = K.pairs(cnt, K.CUT)
    assert res.sample_id == [f"s{q}" for q in range(N)] and res.n == N and res.n_markers == M
    assert res.kin_cutoff == K.CUT and not res.is_dense and i.size > 10
    assert np.array_equal(res.i, i) and np.array_equal(res.j, j) and res.i.dtype == np.int32
    assert np.array_equal(res.kinship, kin) and np.array_equal(res.IBS0, ibs) and np.array_equal(res.n_snp, c5[:, 0])
    rp = res.related_pairs()
    assert rp[0] == (f"s{i[0]}", f"s{j[0]}", float(kin[0]), float(ibs[0])) and len(rp) == i.size
    assert np.array_equal(res.degree(), K.band(kin))
    Kd = res.to_dense()
    assert Kd.shape == (N, N) and (np.diag(Kd) == 0.5).all() and np.array_equal(Kd[i, j], kin) and np.array_equal(Kd, Kd.T)
    assert len(res.related_pairs(0.2)) == int((kin >= 0.2).sum())


def test_driver_sample_order_and_subset(codes):
    full = _fit(codes)
    rng = np.random.default_rng(3)
    order = rng.permutation(N)[:45]
    ids = [f"s{q}" for q in order]
    res = _fit(codes, sample_id=ids)
    assert res.sample_id == ids and res.n == 45
    sub = K.counts(codes[:, order])                        # the caller's order
    i, j, kin, ibs, c5 = K.pairs(sub, K.CUT)
    assert np.array_equal(res.i, i) and np.array_equal(res.j, j)
    assert np.array_equal(res.kinship, kin) and np.array_equal(res.IBS0, ibs) and np.array_equal(res.n_snp, c5[:, 0])
    want = {(min(a, b), max(a, b)) for a, b in zip(order[i].tolist(), order[j].tolist())}
    have = {(int(a), int(b)) for a, b in zip(full.i, full.j)}
    assert want == {pr for pr in have if pr[0] in set(order.tolist()) and pr[1] in set(order.tolist())}


def test_driver_dense_form_and_budget(codes, monkeypatch):
    import saigegds_amd.grm as grm_mod
    import saigegds_amd.king as king_mod
    monkeypatch.setattr(king_mod, "DENSE_BLOCK", 25)       # several blocks, the lower ones mirrored
    res = _fit(codes, kin_cutoff=None)
    cnt = K.counts(codes)
    kin, ibs = K.values(cnt)
    assert res.is_dense and res.kin_cutoff is None and res.i.size == 0
    assert np.array_equal(res.kinship, kin, equal_nan=True) and np.array_equal(res.IBS0, ibs, equal_nan=True)
    assert np.array_equal(res.n_snp, cnt[0]) and res.n_snp.dtype == np.int32
    sparse = _fit(codes)
    i, j, k2, b2 = res.pairs()
    assert np.array_equal(i, sparse.i) and np.array_equal(j, sparse.j) and np.array_equal(k2, sparse.kinship)
    assert unrelated_set(res) == unrelated_set(sparse)
    order = np.random.default_rng(5).permutation(N)[:20]
    sub = _fit(codes, kin_cutoff=None, sample_id=[f"s{q}" for q in order])
    assert np.array_equal(sub.kinship, kin[np.ix_(order, order)], equal_nan=True)
    assert np.array_equal(sub.n_snp, cnt[0][np.ix_(order, order)])
    monkeypatch.setattr(grm_mod, "DENSE_BUDGET_BYTES", 20 * N * N - 1)
    with pytest.raises(ValueError, match="kin_cutoff"):
        _fit(codes, kin_cutoff=None)
    _fit(codes)                                            # (the list of pairs has no such limit)


@pytest.mark.parametrize("ext", [".rds", ".npz"])
@pytest.mark.parametrize("cut", [K.CUT, None])
def test_driver_file_round_trip(codes, tmp_path, ext, cut):
    fn = str(tmp_path / ("king" + ext))
    res = _fit(codes, kin_cutoff=cut, out_fn=fn)
    back = load_king(fn)
    assert back.sample_id == res.sample_id and back.n == res.n and back.n_markers == res.n_markers
    assert back.kin_cutoff == res.kin_cutoff and back.is_dense == res.is_dense
    for k in ("i", "j", "kinship", "IBS0", "n_snp"):
        a, b = getattr(back, k), getattr(res, k)
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if ext == ".rds" and cut is not None:
        from saigegds_amd.rds import read_rds
        r = read_rds(fn)
        assert list(r.names) == ["sample.id", "i", "j", "kinship", "IBS0", "n.snp", "n", "n.markers", "kin.cutoff"]
        assert int(np.asarray(r["i"])[0]) == int(res.i[0]) + 1


def test_driver_refusals(codes):
    with pytest.raises(ValueError, match="RDS or npz"):
        _fit(codes, out_fn="king.txt")
    with pytest.raises(ValueError, match="kin_cutoff"):
        _fit(codes, kin_cutoff=float("nan"))
    with pytest.raises(ValueError, match="unique"):
        _fit(codes, sample_id=["s1", "s1"])


def test_driver_variant_id_passes_through(codes):
    src = K.source(codes)
    ids = np.asarray(src.variant_id)
    keep = ids[::3]
    res = seqFitKING(src, variant_id=keep, verbose=False, operator_factory=K.NumpyKing, **K.FILTER)
    assert res.n_markers == keep.size
    i, j, kin = K.pairs(K.counts(codes[::3]), K.CUT)[:3]
    assert np.array_equal(res.i, i) and np.array_equal(res.j, j) and np.array_equal(res.kinship, kin)
