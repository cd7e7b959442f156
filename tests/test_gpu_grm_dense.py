"""GPU: the explicit GRM (kern_grm_dense.h, host_grm_dense.h: sgx_grm_dense, sgx_grm_sparse) against the long-double
reference of grm_dense_ref.py at the dword (16), tile (16 / 64 / 256) and padding (512) edges, with more than one
FP64 slab and int32 chunk of the screen at M = 140000; its ties to the pinned operator (the diagonal, K b =
crossprod(b)); sparse = thresholded dense, bit for bit and without exclusions, on planted relatives; the screen
bound at a cutoff one ulp either side of a value; and the error returns.

Accuracy bound: 4 E_DENSE scaled units (grm_dense_ref.py), E_DENSE being the worst scaled error of a plain double
g.T @ g / M over the same shapes (test_grm_dense_ref.py)."""
import functools

import numpy as np
import pytest

import grm_dense_ref as D
import grm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

BOUND = 4 * D.E_DENSE
OP_BOUND = 4 * R.E_ORC + 4 * D.E_DENSE
GUARD = -7.25e77
EINVAL, ENOSPACE = -1, -5
SCREEN_SHAPE = (300, 140000)        # 1094 steps of the screen: two folds of its int32 sums into int64, and a rest
SCREEN_SHAPE_CUTOFFS = D.CUTOFFS + (D.EVERYTHING,)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


@functools.lru_cache(maxsize=None)
def _dense(n, m, miss):
    """dense(), diag() and the crossprod of three vectors of one case: computed once, read-only."""
    from saigegds_amd._lib import GrmOperator
    codes, _ = D.case(n, m, miss)
    B = R.vectors(n, R.case_seed(n, m, miss))
    kinds = [R.VECTOR_KINDS.index(k) for k in ("normal", "pm1", "onehot")]
    with GrmOperator(R.pack(codes), n) as op:
        K, diag = op.dense(), op.diag()
        prods = [op.crossprod(B[k]) for k in kinds]
        sparse = {c: op.sparse(c, return_stats=True) for c in SCREEN_SHAPE_CUTOFFS} if (n, m) == SCREEN_SHAPE else {}
    K.setflags(write=False)
    return K, diag, B[kinds], prods, sparse


@pytest.mark.parametrize("c", D.CASES, ids=R.case_id)
def test_dense_against_long_double(c):
    n, m, miss = c
    codes, ref = D.case(*c)
    K, diag, B, prods, _ = _dense(*c)
    e = D.scaled_error(K, ref)                             # (asserts exact zeros where scale_ij == 0)
    print("\n%s scaled error %.4g" % (R.case_id(c), e))
    assert e <= BOUND
    assert np.all(K[n - 1] == 0) and np.all(K[:, n - 1] == 0)           # the all-missing sample
    assert np.array_equal(K, K.T)
    # ties to the pinned operator
    ed = R.scaled_error(np.diag(K), diag.astype(R.LD), np.diag(ref.scale))
    print("diag against sgx_grm_diag: %.4g scaled units" % ed)
    assert ed <= BOUND
    op_ref = R.reference(codes, B)
    Kl = K.astype(R.LD)
    for k in range(B.shape[0]):
        kb = Kl @ B[k].astype(R.LD)
        ek = R.scaled_error(kb, np.asarray(prods[k], dtype=R.LD), op_ref.scale[k])
        print("K b vs crossprod, vector %d: %.4g" % (k, ek))
        assert ek <= OP_BOUND, k


@pytest.mark.parametrize("miss", R.MISS)
def test_sparse_over_several_int32_chunks_of_the_screen(miss):
    """M = 140000 is 1094 steps of the screen: its int32 sums are folded into int64 twice in the loop and once at
    the end, at both missing rates.  sparse = thresholded dense: the same index set, the same bits, sorted."""
    n, m = SCREEN_SHAPE
    assert (m + 511) // 512 * 512 // 128 > 2 * 512
    K, _, _, _, sparse = _dense(n, m, miss)
    nst = (n + 15) // 16
    for c, (i, j, x, st) in sparse.items():
        wi, wj, wx = D.threshold(K, c)
        print("\nmiss %g cutoff %g: %d entries, %d of %d sub-tiles flagged" % (miss, c, i.size, st["subtiles_flagged"],
                                                                             st["subtiles_total"]))
        assert np.array_equal(i, wi) and np.array_equal(j, wj), c
        assert np.array_equal(x.view(np.uint64), wx.view(np.uint64)), c
        assert st["subtiles_total"] == nst * (nst + 1) // 2
        if c == D.EVERYTHING:
            assert st["subtiles_flagged"] == st["subtiles_total"] and i.size == n * (n + 1) // 2
    assert sparse[0.125][3]["subtiles_flagged"] < sparse[0.125][3]["subtiles_total"]


def test_block_placement_and_transpose_window():
    from saigegds_amd._lib import GrmOperator
    n, m, miss = 513, 511, 5e-3
    codes, _ = D.case(n, m, miss)
    K = _dense(n, m, miss)[0]
    with GrmOperator(R.pack(codes), n) as op:
        a = op.dense_block(3, 21, 250, 19)
        b = op.dense_block(250, 19, 3, 21)
        whole = op.dense_block(0, n, 0, n)
        # rectangles that straddle the diagonal off the tile grid: of a tile pair (ti, tj), (tj, ti) one is computed
        strad, strad2 = op.dense_block(100, 200, 37, 364), op.dense_block(37, 364, 100, 200)
        # leading dimension: the gaps are not written
        out = np.full((21, 40), GUARD)
        rc = op._L.sgx_grm_dense(op._h, 3, 21, 250, 19, out.ctypes.data, 40)
    assert rc == 0
    assert np.array_equal(a, K[3:24, 250:269]) and np.array_equal(b, K[250:269, 3:24]) and np.array_equal(b, a.T)
    assert np.array_equal(whole, K)
    assert np.array_equal(strad, K[100:300, 37:401]) and np.array_equal(strad2, K[37:401, 100:300])
    assert np.array_equal(out[:, :19], a) and np.all(out[:, 19:] == GUARD)


@functools.lru_cache(maxsize=None)
def _planted_run(n, m):
    from saigegds_amd._lib import GrmOperator
    p, _ = D.planted(n, m)
    res = {}
    with GrmOperator(R.pack(p.codes), n) as op:
        K = op.dense()
        for c in D.CUTOFFS + (D.EVERYTHING,):
            res[c] = op.sparse(c, return_stats=True)
        again = op.sparse(0.125)
    return K, res, again


@pytest.mark.parametrize("n,m", D.PLANTED)
def test_sparse_is_thresholded_dense(n, m):
    p, ref = D.planted(n, m)
    K, res, again = _planted_run(n, m)
    assert D.scaled_error(K, ref) <= BOUND
    for c, (i, j, x, st) in res.items():
        wi, wj, wx = D.threshold(K, c)
        print("\ncutoff %g: %d entries, %d of %d sub-tiles flagged, s = %d" % (c, i.size, st["subtiles_flagged"],
                                                                              st["subtiles_total"], st["s"]))
        assert np.array_equal(i, wi) and np.array_equal(j, wj), c            # the same set, already sorted
        assert np.array_equal(x.view(np.uint64), wx.view(np.uint64)), c      # bit for bit
        assert st["entries"] == i.size
        nst = (n + 15) // 16
        assert st["subtiles_total"] == nst * (nst + 1) // 2
        if c == D.EVERYTHING:
            assert st["subtiles_flagged"] == st["subtiles_total"] and i.size == n * (n + 1) // 2
    assert res[0.125][3]["subtiles_flagged"] < res[0.125][3]["subtiles_total"]     # the screen did screen
    found = set(zip(res[0.125][0].tolist(), res[0.125][1].tolist()))
    for a, b in [p.dup] + p.parent_child + [p.sibs]:
        assert (min(a, b), max(a, b)) in found, (a, b)
    assert (min(p.disjoint), max(p.disjoint)) not in found
    for a, b in zip(again, res[0.125][:3]):
        assert a.tobytes() == b.tobytes()


def test_bound_is_conservative_one_ulp_either_side():
    from saigegds_amd._lib import GrmOperator
    n, m = D.PLANTED[0]
    p, _ = D.planted(n, m)
    K = _planted_run(n, m)[0]
    a, b = min(p.sibs), max(p.sibs)
    v = K[a, b]
    with GrmOperator(R.pack(p.codes), n) as op:
        for cut, present in ((np.nextafter(v, -np.inf), True), (v, True), (np.nextafter(v, np.inf), False)):
            i, j, x = op.sparse(float(cut))
            wi, wj, wx = D.threshold(K, cut)
            assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(x, wx)
            assert ((a, b) in set(zip(i.tolist(), j.tolist()))) == present, cut


def test_errors_leave_the_output_untouched():
    import ctypes as C
    from saigegds_amd._lib import GrmOperator, SgxGrmSparseStats
    n, m = D.PLANTED[0]
    p, _ = D.planted(n, m)
    K, res, _ = _planted_run(n, m)
    need = res[0.125][0].size
    with GrmOperator(R.pack(p.codes), n) as op:
        L, h = op._L, op._h

        def sparse(cut, cap, size=None):
            size = cap if size is None else size
            i = np.full(size + 8, -77, dtype=np.int32)
            j = np.full(size + 8, -77, dtype=np.int32)
            x = np.full(size + 8, GUARD)
            n_out = C.c_size_t(12345)
            rc = L.sgx_grm_sparse(h, cut, cap, i.ctypes.data, j.ctypes.data, x.ctypes.data, C.byref(n_out),
                                  C.byref(SgxGrmSparseStats()))
            return rc, n_out.value, i, j, x

        rc, k, i, j, x = sparse(0.125, need - 1)
        assert rc == ENOSPACE and k == need
        assert np.all(i[need - 1:] == -77) and np.all(j[need - 1:] == -77) and np.all(x[need - 1:] == GUARD)
        rc, k, i, j, x = sparse(0.125, need)
        assert rc == 0 and k == need and np.array_equal(i[:need], res[0.125][0]) and np.all(x[need:] == GUARD)
        for bad in (float("nan"), float("inf"), float("-inf")):
            rc, k, i, j, x = sparse(bad, need)
            assert rc == EINVAL and np.all(i == -77) and np.all(x == GUARD), bad
        out = np.full((4, 4), GUARD)
        for i0, ni, j0, nj, ld in ((-1, 4, 0, 4, 4), (0, 4, n - 3, 4, 4), (n, 1, 0, 4, 4), (0, 4, 0, 4, 3),
                                   (0, -1, 0, 4, 4)):
            assert L.sgx_grm_dense(h, i0, ni, j0, nj, out.ctypes.data, ld) == EINVAL, (i0, ni, j0, nj, ld)
            assert np.all(out == GUARD)
        assert L.sgx_grm_dense(h, 0, 4, 0, 4, None, 4) == EINVAL
        assert L.sgx_grm_sparse(h, 0.125, need, None, None, None, None, None) == EINVAL
        # the handle stays usable, with or without marker groups, which are ignored
        op.set_groups(np.arange(m) % 3, 3)
        assert np.array_equal(op.dense_block(0, n, 0, n), K)
        i, j, x = op.sparse(0.125)
        assert np.array_equal(i, res[0.125][0]) and np.array_equal(x, res[0.125][2])
