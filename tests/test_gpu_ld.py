"""The device LD kernel (kern_ld.h) against tests/ld_ref.py, bit for bit: the six sums at every sample
count of the case table and the row counts around the 16-row fragment and the 32-row tile, the special rows, garbage
in the padding, a sum over 16 bits, the identities, the block flags and the window ring."""
import numpy as np
import pytest

import ld_cases as LC
import ld_ref as R

pytestmark = pytest.mark.gpu


def _engine(n, bpv, **kw):
    from saigegds_amd._lib import LdEngine
    return LdEngine(n, bpv, **kw)


@pytest.mark.parametrize("n,ma,mb", LC.COUNT_CASES)
def test_counts_bit_for_bit(n, ma, mb):
    """All-missing, monomorphic, disjoint (n = 0) and single-overlap (n = 1) rows are rows 0..5 of each side; the
    stride is 5 bytes over ceil(n/4), with random bytes there and random bits in the last byte's unused fields."""
    ca, cb = LC.random_codes(n, ma, 7 * n + 1), LC.random_codes(n, mb, 7 * n + 2)
    want = R.counts(ca, cb)
    pa, pb = LC.padded(ca, 5, n), LC.padded(cb, 5, n + 1)
    with _engine(n, pa.shape[1]) as eng:
        got = eng.counts(pa, pb)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        # x and y swap with the arguments
        assert np.array_equal(eng.counts(pb, pa), want.transpose(1, 0, 2)[..., [0, 2, 1, 4, 3, 5]])
    from saigegds_amd import ld_counts_2bit
    assert np.array_equal(ld_counts_2bit(R.pack(ca), R.pack(cb), n), want)


def test_sum_over_16_bits():
    n = 70001
    codes = np.full((2, n), 2, dtype=np.uint8)
    with _engine(n, (n + 3) // 4) as eng:
        got = eng.counts(R.pack(codes), R.pack(codes))
    assert got[0, 1].tolist() == [n, 2 * n, 2 * n, 280004, 280004, 280004]
    assert np.array_equal(got, R.counts(codes, codes))


def test_pair_alone_and_inside_a_large_call():
    n = 1025
    ca, cb = LC.random_codes(n, 65, 21), LC.random_codes(n, 65, 22)
    pa, pb = R.pack(ca), R.pack(cb)
    with _engine(n, pa.shape[1]) as eng:
        big = eng.counts(pa, pb)
        for i, j in ((0, 0), (7, 40), (33, 16), (64, 64), (31, 32)):
            assert np.array_equal(eng.counts(pa[i:i + 1], pb[j:j + 1])[0, 0], big[i, j])
    assert np.array_equal(big, R.counts(ca, cb))


def test_diagonal_equals_geno_stats():
    from saigegds_amd._lib import geno_stats_2bit
    n = 257
    c = LC.random_codes(n, 33, 5)
    p = R.pack(c)
    with _engine(n, p.shape[1]) as eng:
        s = eng.counts(p, p)
    nv, ac = geno_stats_2bit(p, n)
    d = np.arange(33)
    assert np.array_equal(s[d, d, 0], nv) and np.array_equal(s[d, d, 1], ac)


def test_block_flags_and_tie():
    codes = LC.ld_source(**LC.FLAG_ROWS)[0]
    n = codes.shape[1]
    p = LC.padded(codes, 3, 9)
    with _engine(n, p.shape[1]) as eng:
        for t in LC.THRESHOLDS:
            eng.reset()
            f0 = eng.block(p[:70], t * t)
            assert f0.shape == (70, 70)
            assert np.array_equal(np.tril(f0, -1), np.tril(R.in_ld(R.counts(codes[:70], codes[:70]), t * t), -1))
            keep = np.arange(0, 70, 3)
            eng.push(keep, 0)
            assert eng.window_len == keep.size
            f1 = eng.block(p[70:150], t * t)
            assert f1.shape == (80, keep.size + 80)
            assert np.array_equal(f1[:, :keep.size], R.in_ld(R.counts(codes[70:150], codes[keep]), t * t))
            assert np.array_equal(np.tril(f1[:, keep.size:], -1),
                                  np.tril(R.in_ld(R.counts(codes[70:150], codes[70:150]), t * t), -1))
            assert f1.any() and not f1.all()
    tie = R.pack(np.array([LC.TIE_Y, LC.TIE_X], dtype=np.uint8))
    lo = float(np.nextafter(0.5, 0))
    with _engine(4, 1) as eng:
        assert eng.block(tie, 0.5 * 0.5)[1, 0] == 0
        assert eng.block(tie, lo * lo)[1, 0] == 1
        eng.block(tie, 0.25)
        eng.push([0], 0)
        assert eng.block(tie[1:], 0.5 * 0.5)[0, 0] == 0 and eng.block(tie[1:], lo * lo)[0, 0] == 1


def test_window_ring_wraps():
    """A window of 256 rows of room, filled, then two pushes that drop from the front: the appended rows wrap round the
    ring, and the columns stay oldest first."""
    codes = LC.ring_codes()
    n, t2 = codes.shape[1], LC.RING["t2"]
    p = R.pack(codes)
    probe = p[:16]
    with _engine(n, p.shape[1]) as eng:
        win = np.zeros(0, dtype=np.int64)
        for lo, hi, keep, drop in ((0, 256, np.arange(256), 0), (256, 400, np.arange(0, 144, 2), 100),
                                   (400, 600, np.arange(1, 200, 3), 60)):
            eng.block(p[lo:hi], t2)
            eng.push(keep, drop)
            win = np.concatenate([win[drop:], lo + keep])
            assert eng.window_len == win.size <= 256
            f = eng.block(probe, t2)
            assert np.array_equal(f[:, :win.size], R.in_ld(R.counts(codes[:16], codes[win]), t2))
        eng.reset()
        assert eng.window_len == 0 and eng.block(probe, t2).shape == (16, 16)


def test_window_grows_while_wrapped():
    """The ring of 256 rows is filled, wrapped by a drop and a push, and then pushed past 256 rows with a drop: it grows
    with its first row in the middle of the old ring, so its rows move in two pieces.  A failed push (over the budget of
    600 rows) leaves the window as it was; then the ring of 512 wraps again and grows to the whole budget."""
    codes = LC.ring_codes()
    n, t2 = codes.shape[1], LC.RING["t2"]
    p = R.pack(codes)
    probe = p[:16]
    with _engine(n, p.shape[1], window_bytes=600 * 64) as eng:       # a budget of 600 rows of one 64-byte unit
        win = np.zeros(0, dtype=np.int64)

        def step(lo, hi, keep, drop):
            nonlocal win
            eng.block(p[lo:hi], t2)
            eng.push(keep, drop)
            win = np.concatenate([win[drop:], lo + keep])

        def check():
            assert eng.window_len == win.size
            f = eng.block(probe, t2)
            assert np.array_equal(f[:, :win.size], R.in_ld(R.counts(codes[:16], codes[win]), t2))

        step(0, 256, np.arange(256), 0)
        step(256, 400, np.arange(0, 144, 2), 100)                     # 228 rows, wrapped: first row at slot 100
        check()
        step(300, 500, np.arange(200), 10)                            # 418 rows: grows from a wrapped ring
        check()
        eng.block(p[0:256], t2)
        with pytest.raises(MemoryError):
            eng.push(np.arange(256), 50)                              # 624 rows: over the budget, nothing changes
        check()
        step(100, 300, np.arange(0, 200, 2), 300)                     # 218 rows in the ring of 512, first row at slot 300
        check()
        step(0, 256, np.arange(256), 0)                               # 474 rows: wrapped
        step(256, 382, np.arange(126), 0)                             # 600 rows: grows wrapped, to the whole budget
        check()


def test_errors_leave_the_handle_usable():
    from saigegds_amd._lib import LD_BLOCK, SgxError, load
    import ctypes as C
    L = load()
    h = C.c_void_p()
    assert L.sgx_ld_create(0, 10, 2, 0, C.byref(h)) == -1            # bytes_per_variant < ceil(n/4)
    c = LC.random_codes(65, LD_BLOCK + 1, 8)
    p = R.pack(c)
    with _engine(65, p.shape[1]) as eng:
        with pytest.raises(SgxError):
            eng.block(p, 0.04)                                        # over the cap
        assert L.sgx_ld_block_2bit(eng._h, None, 1, 0.04, None) == -1
        assert L.sgx_ld_counts_2bit(eng._h, None, 1, None, 1, None) == -1
        with pytest.raises(SgxError):
            eng.push([0], 0)                                          # no block resident
        eng.block(p[:8], 0.04)
        with pytest.raises(SgxError):
            eng.push([3, 2], 0)                                       # not ascending
        with pytest.raises(SgxError):
            eng.push([1], 1)                                          # more to drop than the window holds
        assert np.array_equal(eng.counts(p[:8], p[:8]), R.counts(c[:8], c[:8]))
    with _engine(65, p.shape[1], window_bytes=3 * 64) as eng:        # a budget of three rows
        eng.block(p[:8], 0.04)
        with pytest.raises(MemoryError):
            eng.push([0, 1, 2, 3], 0)
        eng.push([0, 1, 2], 0)
        assert eng.window_len == 3
