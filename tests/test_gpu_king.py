"""sgx_grm_king_counts / sgx_grm_king_pairs (kern_king.h) against tests/king_ref.py: integers and the
bits of kinship / IBS0, with no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import grm_ref as R
import king_ref as K

pytestmark = pytest.mark.gpu

NS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 257)           # sub-tile and tile edges
MS = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2000)   # the MFMA step, the 128-marker step, Gt's 512-marker padding
MISSES = (0.0, 0.05, 0.6)
# every N at three values of M and every M at three values of N; the missing rate cycles through MISSES
_PAIRS = sorted({(n, m) for n in NS for m in (1, 129, 513)} | {(n, m) for m in MS for n in (17, 65, 129)})
CASES = [(n, m, MISSES[k % 3]) for k, (n, m) in enumerate(_PAIRS)]


def make_codes(n, m, miss, seed=0):
    """Random codes [m, n]: allele frequencies U(0.05, 0.95), entries missing at rate ``miss``; where n allows, sample
    n - 1 is all missing and sample n // 2 has no heterozygote."""
    rng = np.random.default_rng([seed, n, m, int(1000 * miss)])
    codes = rng.binomial(2, rng.uniform(0.05, 0.95, m)[:, None], size=(m, n)).astype(np.uint8)
    codes[rng.random((m, n)) < miss] = 3
    if n >= 3:
        codes[:, n - 1] = 3
        col = codes[:, n // 2]
        col[col == 1] = 2
    return codes


def operator(codes):
    from saigegds_amd._lib import GrmOperator
    return GrmOperator(R.pack(codes), codes.shape[1])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n,m,miss", CASES, ids=lambda v: str(v))
def test_counts_whole_square(n, m, miss):
    codes = make_codes(n, m, miss)
    want = K.counts(codes)
    with operator(codes) as op:
        got = op.king_counts(0, n, 0, n)
    assert got.dtype == np.int32 and got.shape == (5, n, n)
    assert np.array_equal(got, want)


def test_many_steps():
    n, m = 129, 70001
    codes = make_codes(n, m, 0.05)
    with operator(codes) as op:
        got = op.king_counts(0, n, 0, n)
        i, j, kin, ibs, cnt = op.king_pairs(-1e300)
    want = K.counts(codes)
    assert np.array_equal(got, want)
    wi, wj, wk, wb, wc = K.pairs(want, -1e300)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(cnt, wc)
    assert same_bits(kin, wk) and same_bits(ibs, wb)


@pytest.fixture(scope="module")
def square():
    n, m = 257, 513
    codes = make_codes(n, m, 0.05, seed=3)
    with operator(codes) as op:
        yield codes, op, op.king_counts(0, n, 0, n)


@pytest.mark.parametrize("i0,ni,j0,nj", [(0, 40, 130, 100), (50, 100, 100, 100), (200, 1, 0, 257), (256, 1, 3, 1),
                                         (63, 67, 1, 129), (100, 157, 0, 64)])
def test_rectangles(square, i0, ni, j0, nj):
    codes, op, full = square
    got = op.king_counts(i0, ni, j0, nj)
    assert np.array_equal(got, full[:, i0:i0 + ni, j0:j0 + nj])
    assert np.array_equal(full, K.counts(codes))
    assert np.array_equal(full, full[[0, 2, 1, 3, 4]].transpose(0, 2, 1))      # (i, j) = (j, i) with hi / hj swapped


def test_rectangle_with_a_wider_ld(square):
    from saigegds_amd._lib import load
    codes, op, full = square
    i0, ni, j0, nj, ld = 60, 70, 120, 33, 40
    out = np.full((5, ni, ld), -7, dtype=np.int32)
    assert load().sgx_grm_king_counts(op._h, i0, ni, j0, nj, out.ctypes.data, ld) == 0
    assert np.array_equal(out[:, :, :nj], full[:, i0:i0 + ni, j0:j0 + nj])
    assert (out[:, :, nj:] == -7).all()


def test_same_samples_same_bits_anywhere():
    """Two samples' five integers and kinship bits do not depend on their indices, their neighbours or N."""
    m = 1000
    base = make_codes(300, m, 0.05, seed=5)
    a, b = base[:, 7].copy(), base[:, 8].copy()
    want = K.counts(np.stack([a, b], axis=1))[:, 0, 1]
    kin_want = K.values(want.reshape(5, 1))[0]
    seen = []
    for n, ia, ib, seed in ((2, 0, 1, 0), (300, 7, 8, 5), (300, 70, 299, 6), (65, 64, 3, 7), (130, 63, 64, 8)):
        codes = make_codes(n, m, 0.3, seed=seed)
        codes[:, ia], codes[:, ib] = a, b
        with operator(codes) as op:
            c = op.king_counts(0, n, 0, n)
            i, j, kin, ibs, cnt = op.king_pairs(-1e300)
        lo, hi = min(ia, ib), max(ia, ib)
        assert np.array_equal(c[:, ia, ib], want)
        assert np.array_equal(c[:, ib, ia], want[[0, 2, 1, 3, 4]])
        k = np.flatnonzero((i == lo) & (j == hi))
        assert k.size == 1
        assert np.array_equal(cnt[k[0]], want if ia < ib else want[[0, 2, 1, 3, 4]])
        assert same_bits(kin[k], kin_want)
        seen.append(kin[k[0]])
    assert len({float(v).hex() for v in seen}) == 1


def test_padding_enters_nothing():
    n = 70
    codes = make_codes(n, 513, 0.05, seed=9)
    wide = np.concatenate([codes, np.full((1024 - 513, n), 3, dtype=np.uint8)])
    with operator(codes) as a, operator(wide) as b:
        ca, cb = a.king_counts(0, n, 0, n), b.king_counts(0, n, 0, n)
    assert np.array_equal(ca, cb) and np.array_equal(ca, K.counts(codes))


@pytest.fixture(scope="module", params=sorted(K.PEDIGREES))
def ped(request):
    n, m = request.param
    p, cnt = K.planted(n, m)
    with operator(p.codes) as op:
        yield p, cnt, op


def test_pairs_on_the_planted_pedigree(ped):
    p, cnt, op = ped
    n = p.codes.shape[1]
    i, j, kin, ibs, c5 = op.king_pairs(K.CUT)
    wi, wj, wk, wb, wc = K.pairs(cnt, K.CUT)
    assert np.array_equal(i, wi) and np.array_equal(j, wj)
    assert {(int(a), int(b)) for a, b in zip(i, j)} == set(p.planted)
    assert np.array_equal(c5, wc) and same_bits(kin, wk) and same_bits(ibs, wb)
    # ... and they are the king_counts-derived values
    from saigegds_amd._lib import king_values
    full = op.king_counts(0, n, 0, n)
    assert np.array_equal(full, cnt)
    fk, fb = king_values(full)
    assert same_bits(kin, fk[i, j]) and same_bits(ibs, fb[i, j]) and np.array_equal(c5, full[:, i, j].T)
    assert K.band(kin).tolist() == [p.planted[(int(a), int(b))] for a, b in zip(i, j)]
    # twice: the same arrays
    again = op.king_pairs(K.CUT)
    for x, y in zip((i, j, c5), (again[0], again[1], again[4])):
        assert np.array_equal(x, y)
    assert same_bits(kin, again[2]) and same_bits(ibs, again[3])


def test_pairs_cutoff_is_inclusive(ped):
    p, cnt, op = ped
    wi, wj, wk, _, _ = K.pairs(cnt, K.CUT)
    k = int(np.argmin(wk))
    own = float(wk[k])
    i, j = op.king_pairs(own)[:2]
    assert (int(wi[k]), int(wj[k])) in set(zip(i.tolist(), j.tolist()))
    assert np.array_equal(i, K.pairs(cnt, own)[0])
    i2, j2 = op.king_pairs(float(np.nextafter(own, np.inf)))[:2]
    assert (int(wi[k]), int(wj[k])) not in set(zip(i2.tolist(), j2.tolist()))
    assert i2.size == i.size - int((wk == own).sum())


def test_pairs_below_every_value_lists_all_defined_pairs(ped):
    p, cnt, op = ped
    n = p.codes.shape[1]
    i, j, kin, ibs, c5 = op.king_pairs(-1e300)
    wi, wj, wk, wb, wc = K.pairs(cnt, -1e300)
    iu, ju = np.triu_indices(n, 1)
    assert wi.size == int((np.minimum(cnt[1], cnt[2])[iu, ju] > 0).sum())
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(c5, wc)
    assert same_bits(kin, wk) and same_bits(ibs, wb) and not np.isnan(kin).any()


def test_nan_pairs_never_appear():
    codes = make_codes(40, 300, 0.05, seed=11)             # sample 39 all missing, sample 20 without a heterozygote
    with operator(codes) as op:
        i, j, kin = op.king_pairs(-1e300)[:3]
    assert not np.isnan(kin).any()
    assert not ((i == 39) | (j == 39) | (i == 20) | (j == 20)).any()
    assert i.size == 38 * 37 // 2


def _raw_pairs(op, cutoff, cap, with_counts=True):
    from saigegds_amd._lib import SgxGrmKingStats, load
    i, j = np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32)
    kin, ibs = np.full(cap, -7.0), np.full(cap, -7.0)
    c5 = np.full((cap, 5), -7, dtype=np.int32)
    n_out, st = C.c_size_t(12345), SgxGrmKingStats()
    rc = load().sgx_grm_king_pairs(op._h, cutoff, cap, i.ctypes.data, j.ctypes.data, kin.ctypes.data, ibs.ctypes.data,
                                   c5.ctypes.data if with_counts else None, C.byref(n_out), C.byref(st))
    return rc, int(n_out.value), (i, j, kin, ibs, c5), st.as_dict()


def test_pairs_enospace_then_success(ped):
    from saigegds_amd._lib import ENOSPACE
    p, cnt, op = ped
    want = K.pairs(cnt, K.CUT)
    n_pairs = want[0].size
    rc, n_out, bufs, st = _raw_pairs(op, K.CUT, n_pairs - 1)
    assert rc == ENOSPACE and n_out == n_pairs and st["pairs"] == n_pairs
    assert all((b == -7).all() for b in bufs)
    rc, n_out, bufs, st = _raw_pairs(op, K.CUT, n_pairs, with_counts=False)
    assert rc == 0 and n_out == n_pairs and st["tiles"] > 0 and st["ms_kernel"] > 0
    assert np.array_equal(bufs[0], want[0]) and np.array_equal(bufs[1], want[1]) and same_bits(bufs[2], want[2])
    assert (bufs[4] == -7).all()                           # (no counts asked for)
    got = op.king_pairs(K.CUT, cap=1)                      # the wrapper retries once with the reported size
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[4], want[4])


def test_errors_leave_outputs_untouched(square):
    from saigegds_amd._lib import load
    codes, op, _ = square
    L, n = load(), codes.shape[1]
    out = np.full((5, 8, 8), -7, dtype=np.int32)
    for args in ((-1, 8, 0, 8, 8), (0, 8, n - 7, 8, 8), (n - 7, 8, 0, 8, 8), (0, 8, 0, 8, 7), (0, -1, 0, 8, 8)):
        assert L.sgx_grm_king_counts(op._h, *args[:4], out.ctypes.data, args[4]) == -1
    assert L.sgx_grm_king_counts(op._h, 0, 8, 0, 8, None, 8) == -1
    assert (out == -7).all()
    for cutoff in (float("nan"), float("inf"), float("-inf")):
        rc, n_out, bufs, _ = _raw_pairs(op, cutoff, 16)
        assert rc == -1 and n_out == 12345 and all((b == -7).all() for b in bufs)
    i = np.full(4, -7, dtype=np.int32)
    n_out = C.c_size_t(0)
    assert L.sgx_grm_king_pairs(op._h, 0.1, 4, i.ctypes.data, None, None, None, None, C.byref(n_out), None) == -1
    assert L.sgx_grm_king_pairs(op._h, 0.1, 4, i.ctypes.data, i.ctypes.data, None, None, None, None, None) == -1
    assert (i == -7).all()


def test_other_entries_of_the_handle_unchanged():
    n, m = 257, 2000
    codes = make_codes(n, m, 0.05, seed=13)
    B = np.random.default_rng(1).standard_normal((3, n))
    with operator(codes) as op:
        s0, p0 = op.sparse(0.05), op.crossprod_many(B)
        op.king_pairs(-1e300)
        op.king_counts(0, n, 0, n)
        s1, p1 = op.sparse(0.05), op.crossprod_many(B)
    assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1]) and same_bits(s0[2], s1[2])
    assert same_bits(p0, p1)
