"""sgx_ds_block_firth (DosageBlock.firth, kern_firth_ds.h) on the device: rows of hard calls against sgx_firth_2bit bit
for bit, true dosages against the long-double reference of tests/firth_ds_ref.py at the parity rule of DESIGN.md 9
(1e-10 relative on beta and SE, the NaN pattern and converged exact), lists beyond the LDS part, independence of
position, alignment, order and call, the packed load, the iteration limit, the error paths and the handle's memory.
Models and hard-call rows are those of tests/test_gpu_firth.py."""
import numpy as np
import pytest

import firth_ds_ref as D
import firth_ref as R
from skat_ds_ref import flip_mean
from test_gpu_firth import NROW, _case, _model, _same, check

pytestmark = pytest.mark.gpu
NS = [1, 3, 15, 17, 255, 257, 1000, 1027]
DTYPES = {"u8": np.uint8, "i32": np.int32, "f64": np.float64}
NA_INT = np.iinfo(np.int32).min
MAXIT = 150       # tests 2 and 3: a single sample with g = 0.03 at mu = 1e-4 has beta ~ 340, 68 capped steps from 0
_cache = {}


def _as_dosage(codes, dtype):
    """Hard calls (3 = missing) as dosage rows of ``dtype``."""
    if dtype == np.float64:
        return np.where(codes == 3, np.nan, codes.astype(np.float64))
    return np.where(codes == 3, 0xFF if dtype == np.uint8 else NA_INT, codes.astype(np.int64)).astype(dtype)


def _firth(sc, rows, var_idx, flip, mean, **kw):
    with sc.dosage_block(rows.dtype, rows.shape[0]) as blk:
        blk.load(rows)
        return blk.firth(var_idx, flip, mean, **kw)


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("n", NS)
def test_1_hard_calls_as_dosages_equal_the_2bit_kernel(n, kind):
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import unpack_dosage_2bit
    sm, packed, lut, ref = _case(n)
    rows = _as_dosage(unpack_dosage_2bit(packed, n), DTYPES[kind])
    flip, mean = (lut[:, 0] == 2).astype(np.uint8), lut[:, 3].copy()
    assert np.isnan(mean[6]) and mean[5] == 0                   # the NaN-mean row and the monomorphic row
    with Scanner(sm) as sc:
        want = sc.firth_2bit(packed, lut)
        got = _firth(sc, rows, np.arange(NROW), flip, mean)
    assert _same(got, want), (got - want, got[:, 2], want[:, 2])  # all four columns, the iteration count included
    check(got, ref, f"N={n} {kind}")
    assert np.isnan(got[5, 0]) and np.array_equal(got[6], [np.nan, np.nan, 0, 0], equal_nan=True)


def _true_rows(n):
    """f64 rows: [0] imputed-like, every sample in (0, 0.05]; [1] a few fractional carriers; [2] all carriers cases at
    mu ~ 1e-4; [3] alt-major with NaN missing (flipped); [4] all zeros; [5] a good row whose mean is NaN.  u8: one row of
    byte values 0..5 and 0xFF.  -> (f64 rows, flip, mean, u8 row [1, n], its flip, its mean)."""
    rng = np.random.default_rng(SEED.get(n, 500 + n))
    x = np.zeros((6, n))
    x[0] = 0.05 * (1 - 0.5 * rng.random(n))                      # (0.025, 0.05]: one sample alone at mu = 1e-4 has beta < 4096 / 10
    car = rng.permutation(n)[:max(1, min(6, n // 2))]
    x[1, car] = rng.uniform(0.2, 1.9, car.size)
    cases_rare = np.flatnonzero(np.arange(n) % 10 == 0)
    pick = cases_rare[:max(1, min(7, cases_rare.size))]
    x[2, pick] = rng.uniform(0.4, 1.0, pick.size)
    x[3] = 2 - rng.choice([0.0, 0.25, 1.0, 1.5], n, p=[0.6, 0.1, 0.25, 0.05]) * rng.uniform(0.5, 1, n)
    x[3, rng.random(n) < 0.03] = np.nan
    if n > 3:
        x[3, 1] = np.nan
    x[5] = rng.choice([0.0, 0.5, 1.25], n, p=[0.7, 0.2, 0.1])
    flip, mean = flip_mean(x)
    mean[5] = np.nan
    b = rng.choice(np.array([0, 1, 2, 3, 4, 5, 0xFF], dtype=np.uint8), (1, n), p=[0.5, 0.15, 0.1, 0.08, 0.07, 0.05, 0.05])
    bflip, bmean = flip_mean(b)
    return x, flip, mean, b, bflip, bmean


SEED = {3: 517}   # N -> seed of its rows where 500 + N does not meet test 2's preconditions (checked on the CPU)


def _true_inputs(n):
    if ("in", n) not in _cache:
        _cache["in", n] = (_model(n),) + _true_rows(n)
    return _cache["in", n]


def _true_case(n):
    if n not in _cache:
        sm, x, flip, mean, b, bflip, bmean = _true_inputs(n)
        _cache[n] = (sm, x, flip, mean, D.firth_ds_ref(sm, x, flip, mean), b, bflip, bmean, D.firth_ds_ref(sm, b, bflip, bmean))
    return _cache[n]


def _preconditions(sm, rows, flip, mean, ref, what):
    """Every informative row's reference |beta| >= 1e-3, and the kernel's iteration restated in float64 numpy converges on
    its list within REL_TOL of the long-double root: what the device is then asked for is what the arithmetic can give."""
    from conftest import REL_TOL
    mu, y = np.asarray(sm.mu), np.asarray(sm.y)
    for j in np.flatnonzero(ref[:, 3] == 1):
        b, se, it, ok = R.newton_f64(*D.ds_list(rows[j], flip[j], mean[j], mu, y), maxit=MAXIT)
        assert abs(ref[j, 0]) >= 1e-3 and ok, (what, j, ref[j], b, it)
        assert abs(b - ref[j, 0]) <= REL_TOL * abs(ref[j, 0]) and abs(se - ref[j, 1]) <= REL_TOL * ref[j, 1], (what, j, b, se, ref[j])


@pytest.mark.parametrize("n", NS)
def test_2_true_dosages_against_the_reference(n):
    from saigegds_amd._lib import Scanner
    sm, x, flip, mean, ref, b, bflip, bmean, bref = _true_case(n)
    _preconditions(sm, x, flip, mean, ref, f"N={n} f64")
    _preconditions(sm, b, bflip, bmean, bref, f"N={n} u8")
    assert flip[3] == 1 and flip[0] == 0 and np.isnan(ref[4, 0]) and np.isnan(ref[5, 0])
    if n >= 15:
        assert np.all(ref[:4, 3] == 1) and bref[0, 3] == 1
    if n >= 255:
        assert ref[2, 0] > 9                                     # all carriers cases at mu ~ 1e-4: the step cap at work
    with Scanner(sm) as sc:
        got = _firth(sc, x, np.arange(6), flip, mean, maxit=MAXIT)
        gb = _firth(sc, b, [0], bflip, bmean, maxit=MAXIT)
    check(got, ref, f"N={n} f64")
    check(gb, bref, f"N={n} u8")
    assert np.array_equal(got[5], [np.nan, np.nan, 0, 0], equal_nan=True)          # a NaN mean: no iteration


def test_3_lists_beyond_the_lds_part():
    """N = 50 000: the imputed-like row lists every sample (checked against the reference, with the two rare rows), the
    alt-major row and the u8 row most of them (a row alone gives their bits again)."""
    from saigegds_amd._lib import Scanner
    sm, x, flip, mean, b, bflip, bmean = _true_inputs(50_000)
    mu, y = np.asarray(sm.mu), np.asarray(sm.y)
    assert D.ds_list(x[0], flip[0], mean[0], mu, y)[0].size == 50_000
    assert D.ds_list(x[3], flip[3], mean[3], mu, y)[0].size > 4 * 2048 and D.ds_list(b[0], bflip[0], bmean[0], mu, y)[0].size > 4 * 2048
    ref = D.firth_ds_ref(sm, x[:3], flip[:3], mean[:3])
    _preconditions(sm, x[:3], flip[:3], mean[:3], ref, "N=50000 f64")
    with Scanner(sm) as sc:
        got = _firth(sc, x, np.arange(6), flip, mean, maxit=MAXIT)
        alone = _firth(sc, x[3:4], [0], flip[3:4], mean[3:4], maxit=MAXIT)
        gb = _firth(sc, b, [0, 0], np.repeat(bflip, 2), np.repeat(bmean, 2), maxit=MAXIT)
    check(got[:3], ref, "N=50000 f64")
    assert got[3, 3] == 1 and _same(got[3], alone[0]) and gb[0, 3] == 1 and _same(gb[0], gb[1])


def test_3_position_alignment_order_and_call():
    """N = 1027, u8: a row's start in the block takes every alignment as its index goes up; rows 0, 1 and 5 hold the
    same values."""
    from saigegds_amd._lib import Scanner
    n = 1027
    sm = _case(n)[0]
    rng = np.random.default_rng(77)
    rows = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), (6, n), p=[0.6, 0.28, 0.1, 0.02])
    rows[1] = rows[5] = rows[0]
    flip, mean = flip_mean(rows)
    with Scanner(sm) as sc, sc.dosage_block(np.uint8, 6) as blk:
        blk.load(rows)
        full = blk.firth(np.arange(6), flip, mean)
        assert np.all(full[:, 3] == 1)
        assert _same(full[0], full[1]) and _same(full[0], full[5])                     # block rows 0, 1 and 5
        assert _same(full, blk.firth(np.arange(6), flip, mean))                         # two calls in a row
        assert _same(full[::-1], blk.firth(np.arange(6)[::-1], flip[::-1], mean[::-1]))  # reversed
        idx = np.array([4, 4, 0, 5, 4, 2, 2])
        assert _same(full[idx], blk.firth(idx, flip[idx], mean[idx]))                   # repeated, any order
        for j in range(6):                                                              # a row alone
            assert _same(full[j], blk.firth([j], flip[j:j + 1], mean[j:j + 1])[0]), j
        with sc.dosage_block(np.uint8, 1) as one:                                       # ... and alone in a block
            one.load(rows[3:4])
            assert _same(full[3], one.firth([0], flip[3:4], mean[3:4])[0])
    check(full, D.firth_ds_ref(sm, rows, flip, mean), "N=1027 u8")


def test_3_more_rows_than_the_grid():
    """3 000 rows at N = 257 through one call and one by one."""
    from saigegds_amd._lib import Scanner
    n, m = 257, 3000
    sm = _case(n)[0]
    rng = np.random.default_rng(9)
    f = rng.choice([0.003, 0.02, 0.1, 0.3, 0.7], m)[:, None]
    u = rng.random((m, n))
    rows = ((u < f * f).astype(np.float64) + (u < 1 - (1 - f) ** 2)) * (1 - rng.integers(0, 17, (m, n)) / 64.0)   # fractional carriers
    rows[rng.random((m, n)) < 0.01] = np.nan
    flip, mean = flip_mean(rows)
    with Scanner(sm) as sc, sc.dosage_block(np.float64, m) as blk:
        blk.load(rows)
        full = blk.firth(np.arange(m), flip, mean)
        alone = np.concatenate([blk.firth([j], flip[j:j + 1], mean[j:j + 1]) for j in range(m)])
    assert _same(full, alone)
    conv = full[:, 3] == 1
    assert conv.any() and np.all(np.isfinite(full[conv, :2])) and np.all(np.isnan(full[~conv, 1]))


def test_4_packed_load():
    """load_packed of a dPackedReal16 form == load of its decoded float64 rows."""
    import packed_ds_cases as P
    from saigegds_amd._lib import Scanner
    n, m, cls = 1000, 12, "dPackedReal16"
    sm = _case(n)[0]
    scale, offset = P.DYADIC[cls]
    raw = P.stored_rows(cls, P.dosages(m, n, seed=5), scale, offset)
    wide, sel = P.widen(raw, 1103, seed=6)
    dec = P.decode(raw, cls, scale, offset)
    with Scanner(sm) as sc, sc.dosage_block(np.float64, m) as blk:
        nv, s, _ = blk.load_packed(wide, cls, scale, offset, sel)
        flip, mean = (s > nv).astype(np.uint8), np.where(s > nv, 2 - s / np.maximum(nv, 1), s / np.maximum(nv, 1))
        mean[nv == 0] = np.nan
        a = blk.firth(np.arange(m), flip, mean)
        nv2, s2, _ = blk.load(dec)
        assert np.array_equal(nv, nv2) and np.array_equal(s, s2)
        b = blk.firth(np.arange(m), flip, mean)
    assert _same(a, b) and np.isnan(a[1, 0]) and (a[:, 3] == 1).sum() >= m - 2         # (row 1 is all missing)


def test_5_iteration_limit():
    from saigegds_amd._lib import Scanner
    sm, x, flip, mean, ref, *_ = _true_case(1000)
    with Scanner(sm) as sc, sc.dosage_block(np.float64, 6) as blk:
        blk.load(x)
        idx = np.arange(6)
        full = blk.firth(idx, flip, mean)
        j = int(np.argmax(np.where(full[:, 3] == 1, full[:, 2], 0)))                    # the converged row that took longest
        need = int(full[j, 2])
        assert full[j, 3] == 1 and need >= 3
        short = blk.firth(idx, flip, mean, maxit=need - 1)
        one = blk.firth(idx, flip, mean, maxit=1)
    assert short[j, 3] == 0 and np.isnan(short[j, 1]) and np.isfinite(short[j, 0]) and short[j, 2] == need - 1
    done = full[:, 2] <= need - 1
    assert done.any() and _same(short[done], full[done])                               # the other rows untouched
    info = ~np.isnan(full[:, 0])
    assert np.all(one[info, 3] == 0) and np.all(np.isnan(one[:, 1])) and np.all(one[info, 2] == 1)


def test_6_refusals_leave_handle_and_block_usable():
    """Every refusal that can be reached from one process on one device (a twin handle and a second device cannot)."""
    from saigegds_amd._lib import Scanner, load
    from test_gpu_skat import _model as skat_model
    sm, x, flip, mean, ref, *_ = _true_case(1000)
    L = load()
    idx = np.arange(6, dtype=np.int32)
    o = np.zeros((6, 4))

    def p(a):
        return a.ctypes.data

    ok = (6, p(idx), p(flip), p(mean), 50, p(o))
    with Scanner(sm) as sc, sc.dosage_block(np.float64, 6) as blk, sc.dosage_block(np.float64, 6) as empty:
        blk.load(x)
        h, b = sc._h, blk._b
        assert L.sgx_ds_block_firth(None, b, *ok) == -1 and L.sgx_ds_block_firth(h, None, *ok) == -1
        for i in (1, 2, 3, 5):                                                          # a NULL buffer
            args = list(ok)
            args[i] = None
            assert L.sgx_ds_block_firth(h, b, *args) == -1 and b"NULL buffer" in L.sgx_last_error(), i
        for bad in (0, -3):
            assert L.sgx_ds_block_firth(h, b, 6, p(idx), p(flip), p(mean), bad, p(o)) == -1 and b"maxit" in L.sgx_last_error()
        assert L.sgx_ds_block_firth(h, empty._b, *ok) == -1 and b"nothing loaded" in L.sgx_last_error()
        for bad in (6, -1):
            out = idx.copy()
            out[2] = bad
            assert L.sgx_ds_block_firth(h, b, 6, p(out), p(flip), p(mean), 50, p(o)) == -1
            assert b"outside the block" in L.sgx_last_error()
        with Scanner(_model(257)) as other, other.dosage_block(np.float64, 2) as alien:  # another n_samp
            alien.load(np.zeros((2, 257)))
            assert L.sgx_ds_block_firth(h, alien._b, *ok) == -1 and b"Invalid length of dosages" in L.sgx_last_error()
        with Scanner(skat_model(1000, "quantitative")) as sq, sq.dosage_block(np.float64, 6) as qb:
            qb.load(x)
            assert L.sgx_ds_block_firth(sq._h, qb._b, *ok) == -1 and b"binary" in L.sgx_last_error()
            assert qb.scan()[1].shape == (6,)
        assert L.sgx_ds_block_firth(h, b, 0, None, None, None, 50, None) == 0           # no rows: nothing to do
        assert not o.any()                                                              # nothing was written
        check(blk.firth(idx, flip, mean), ref, "after the refusals")                    # the checked bits
        out, valid = blk.scan()                                                         # the handle still scans
        assert valid.shape == (6,) and np.isfinite(out[valid != 0, 5]).all()


def test_7_memory_returns():
    from saigegds_amd._lib import Scanner, live_bytes
    start = live_bytes()
    sm, x, flip, mean, *_ = _true_inputs(50_000)
    sc = Scanner(sm)
    blk = sc.dosage_block(np.float64, 2)
    blk.load(x[:2])
    before = live_bytes()
    blk.firth([0, 1], flip[:2], mean[:2])
    assert live_bytes() > before                              # the scratch of the long lists, allocated on first use
    held = live_bytes()
    blk.firth([1, 0], flip[1::-1], mean[1::-1])
    assert live_bytes() == held
    blk.close()
    sc.close()
    assert live_bytes() == start


def test_1_an_odd_count_of_entries_at_odd_n():
    """7 entries, not in block order, of a u8 block at N = 1027: the means, the results, the index list and the flips
    each end off a 16-byte boundary, and each table still starts on one.  Against the reference of test 1."""
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import unpack_dosage_2bit
    n = 1027
    sm, packed, lut, ref = _case(n)
    rows = _as_dosage(unpack_dosage_2bit(packed, n), np.uint8)
    flip, mean = (lut[:, 0] == 2).astype(np.uint8), lut[:, 3].copy()
    idx = np.array([7, 0, 4, 2, 6, 3, 1], dtype=np.int32)
    with Scanner(sm) as sc:
        got = _firth(sc, rows, idx, flip[idx], mean[idx])
    check(got, ref[idx], f"N={n} u8, 7 entries")
