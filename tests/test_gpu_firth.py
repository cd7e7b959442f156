"""sgx_firth_2bit(_dev) on the device (kern_firth.h) against the long-double reference of tests/firth_ref.py at the
parity rule of DESIGN.md 9 (1e-10 relative on beta and SE, converged exact), determinism bit for bit, the iteration
limit, the error paths and the handle's memory.

Models: the synthetic one of the SKAT / cond GPU tests (test_gpu_skat._model) from N = 255 up; below that it cannot be
made (N = 1: a singular fit; N = 3: fitted means of 1e-23), so an intercept-only model is written down.  In both, every
5th sample gets a fitted mean near 1e-4 and every 10th of all is a case there: the rows whose carriers are all cases
at mu ~ 1e-4 (beta ~ 11: the step cap and the bracket at work) are made of those."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import firth_ref as R

pytestmark = pytest.mark.gpu
_cache = {}
NROW = 8


def _model(n):
    from saigegds_amd.nullmod import NullModel, init_nullmod
    if n >= 255:
        from test_gpu_skat import _model as skat_model
        sm = skat_model(n)
        mu, y = np.array(sm.mu), np.array(sm.y)
    else:
        rng = np.random.default_rng(n)
        mu, y = rng.uniform(0.05, 0.6, n), (rng.random(n) < 0.4).astype(np.float64)
        X, V = np.ones((n, 1)), mu * (1 - mu)
        mod = NullModel(trait_type="binary", tau=np.array([1.0, 0.0]), fitted_values=mu, sample_id=[f"s{i}" for i in range(n)],
                        var_ratio=np.array([0.94]), y=y, V=V, X1=X, XV=(X * V[:, None]).T, XXVX_inv=X / V.sum())
        sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, 0.94)
    i = np.arange(n)
    rare = i % 5 == 0
    mu[rare] = 1e-4 * (1 + i[rare] / n)
    y[rare] = (i[rare] % 10 == 0)
    return replace(sm, mu=mu, y=y, y_mu=y - mu, mu2=mu * (1 - mu))


def _tables(codes):
    from saigegds_amd import firth
    num = (codes < 3).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        af = np.where(codes < 3, codes, 0).sum(axis=1) / (2.0 * num)
    return firth.firth_tables(af)[0]


def _rows(n, sm):
    """The issue's rows: [0] one carrier, [1] all carriers cases at mu ~ 1e-4, [2] all carriers controls, [3] 2 % missing,
    [4] alt-major with missing codes, [5] monomorphic, [6] a good row with a NaN table, [7] a good row."""
    rng = np.random.default_rng(100 + n)
    y = np.asarray(sm.y)
    codes = np.zeros((NROW, n), dtype=np.uint8)
    codes[0, n // 2] = 1
    cases_rare = np.flatnonzero((np.arange(n) % 10 == 0))
    codes[1, cases_rare[:max(1, min(7, cases_rare.size))]] = 1
    ctrl = np.flatnonzero(y == 0)[::3]
    codes[2, ctrl] = 1 + (np.arange(ctrl.size) % 4 == 0)
    codes[3] = rng.choice([0, 1, 2], n, p=[0.64, 0.32, 0.04])
    codes[3, rng.random(n) < 0.02] = 3
    if n > 3:
        codes[3, 1] = 3
    codes[4] = rng.choice([0, 1, 2], n, p=[0.04, 0.32, 0.64])
    codes[4, rng.random(n) < 0.02] = 3
    codes[6] = rng.choice([0, 1, 2], n, p=[0.81, 0.18, 0.01])
    codes[7] = rng.choice([0, 1, 2], n, p=[0.49, 0.42, 0.09])
    lut = _tables(codes)
    lut[6, 3] = np.nan
    return codes, lut


def _case(n):
    if n not in _cache:
        from saigegds_amd.gds import pack_dosage_2bit
        sm = _model(n)
        codes, lut = _rows(n, sm)
        packed = pack_dosage_2bit(codes)
        _cache[n] = (sm, packed, lut, R.firth_ref(sm, packed, lut))
    return _cache[n]


def check(out4, ref, what):
    """1e-10 relative on beta and SE, the NaN pattern and converged exact."""
    from conftest import REL_TOL
    assert out4.shape == ref.shape, what
    for c, name in ((0, "beta"), (1, "SE")):
        assert np.array_equal(np.isnan(out4[:, c]), np.isnan(ref[:, c])), f"{what}: NaN pattern of {name}: {out4[:, c]} / {ref[:, c]}"
        ok = ~np.isnan(ref[:, c])
        err = np.abs(out4[ok, c] - ref[ok, c]) / np.abs(ref[ok, c])
        print(f"{what}: {name} off by {float(err.max()) if err.size else 0.0:.3g} relative at worst, iterations {out4[:, 2]}")
        assert np.all(err <= REL_TOL), f"{what}: {name} {err}"
    assert np.array_equal(out4[:, 3], ref[:, 3]), f"{what}: converged {out4[:, 3]} / {ref[:, 3]}"


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 255, 257, 1000, 1027])
def test_rows_against_the_reference(n, pad):
    from saigegds_amd._lib import Scanner
    sm, packed, lut, ref = _case(n)
    if pad:
        packed = np.concatenate([packed, np.full((packed.shape[0], pad), 0xFF, dtype=np.uint8)], axis=1)
        if n % 4:
            packed[:, (n + 3) // 4 - 1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)      # codes beyond sample N - 1 in its last byte
    with Scanner(sm) as sc:
        out4 = sc.firth_2bit(packed, lut)
    check(out4, ref, f"N={n} pad={pad}")
    assert np.isnan(ref[5, 0]) and np.isnan(ref[6, 0]) and ref[5, 3] == 0           # monomorphic, NaN table
    if n >= 255:
        assert np.all(ref[[0, 1, 2, 3, 4, 7], 3] == 1)
        assert ref[1, 0] > 9 and ref[2, 0] < 0, ref[:, 0]


def test_a_list_that_does_not_fit_lds():
    """N = 50 000: the 2 % row and the alt-major row (flipped: the samples that are not homozygous alt, 36 %) list more
    than the 4096 entries LDS holds, the rare rows fewer; the alt-major row read with the table of the OTHER orientation
    (not a table the driver makes, but one the entry takes) lists nearly every sample."""
    from saigegds_amd._lib import Scanner
    sm, packed, lut, ref = _case(50_000)
    mu, y = np.asarray(sm.mu), np.asarray(sm.y)
    nnz = [g.size for g, _, _ in R.row_lists(packed, lut, mu, y)]
    assert lut[4, 0] == 2 and nnz[4] > 4 * 4096 and nnz[3] > 4096 > nnz[1]
    alt = np.array([[0.0, 1.0, 2.0, 2 - lut[4, 3]]])
    assert next(R.row_lists(packed[4:5], alt, mu, y))[0].size > 47_500
    ref_alt = R.firth_ref(sm, packed[4:5], alt)
    with Scanner(sm) as sc:
        out4 = sc.firth_2bit(packed, lut)
        again = sc.firth_2bit(packed[4:5], lut[4:5])
        out_alt = sc.firth_2bit(packed[4:5], alt)
    check(out4, ref, "N=50000")
    check(out_alt, ref_alt, "N=50000, nearly every sample listed")
    assert np.array_equal(again[0], out4[4])


@pytest.fixture(scope="module")
def many():
    """3 000 rows at N = 257 (more rows than the grid): frequencies from singletons to alt-major, 1 % missing."""
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 257, 3000
    sm = _case(n)[0]
    rng = np.random.default_rng(9)
    f = rng.choice([0.003, 0.02, 0.1, 0.3, 0.7], m)[:, None]
    u = rng.random((m, n))
    codes = ((u < f * f).astype(np.uint8) + (u < 1 - (1 - f) ** 2)).astype(np.uint8)
    codes[rng.random((m, n)) < 0.01] = 3
    return sm, pack_dosage_2bit(codes), _tables(codes)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_bits_do_not_depend_on_position_order_or_call(many):
    import torch
    from saigegds_amd._lib import Scanner
    sm, packed, lut = many
    m = packed.shape[0]
    with Scanner(sm) as sc:
        full = sc.firth_2bit(packed, lut)
        assert _same(full, sc.firth_2bit(packed, lut))                               # two calls
        assert _same(full[::-1], sc.firth_2bit(packed[::-1], lut[::-1]))               # reversed order
        for j in (0, 1, 511, 512, 513, m - 1):                                        # a row alone, through the host entry
            assert _same(sc.firth_2bit(packed[j:j + 1], lut[j:j + 1])[0], full[j]), j
        stride = sc.row_stride()
        rows = torch.zeros((m, stride), dtype=torch.uint8)
        rows[:, :packed.shape[1]] = torch.from_numpy(packed)
        rows, tl = rows.cuda(), torch.from_numpy(lut).cuda()
        o, alone = (torch.full((m, 4), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        sc.firth_2bit_dev(rows.data_ptr(), stride, m, tl.data_ptr(), o.data_ptr())
        for j in range(m):                                                            # EVERY row alone: a call of one row each
            sc.firth_2bit_dev(rows.data_ptr() + j * stride, stride, 1, tl.data_ptr() + 32 * j, alone.data_ptr() + 32 * j)
        sc.sync()
        assert _same(o.cpu().numpy(), full)                                           # the device entry
        assert _same(alone.cpu().numpy(), full)
    conv = full[:, 3] == 1
    print(f"{int(conv.sum())} of {m} rows converged, at most {int(full[conv, 2].max())} iterations")
    info = ~np.isnan(full[:, 0])
    # (a row whose U* has a near-double root below its root crawls on Fisher steps and runs out of iterations: row 2342)
    assert conv.sum() > 0.95 * info.sum() and np.all(np.isfinite(full[conv, :2]))
    assert np.all(np.isnan(full[~conv, 1])) and np.all(full[info & ~conv, 2] == 50)


def test_iteration_limit(many):
    from saigegds_amd._lib import Scanner
    sm, packed, lut = many
    with Scanner(sm) as sc:
        full = sc.firth_2bit(packed[:50], lut[:50])
        j = int(np.argmax(np.where(full[:, 3] == 1, full[:, 2], 0)))                  # the converged row that took longest
        assert full[j, 3] == 1 and full[j, 2] >= 3
        need = int(full[j, 2])
        short = sc.firth_2bit(packed[:50], lut[:50], maxit=need - 1)
        one = sc.firth_2bit(packed[:50], lut[:50], maxit=1)
    assert short[j, 3] == 0 and np.isnan(short[j, 1]) and np.isfinite(short[j, 0]) and short[j, 2] == need - 1
    done = full[:, 2] <= need - 1
    assert done.any() and _same(short[done], full[done])                             # the other rows untouched
    info = ~np.isnan(full[:, 0])
    assert np.all(one[info, 3] == 0) and np.all(np.isnan(one[:, 1])) and np.all(one[info, 2] == 1)


def test_refusals_leave_the_handle_usable():
    from saigegds_amd._lib import Scanner, SgxError, load
    from test_gpu_skat import _model as skat_model
    sm, packed, lut, ref = _case(1000)
    L = load()
    with Scanner(skat_model(1000, "quantitative")) as sq:
        with pytest.raises(SgxError, match="binary"):
            sq.firth_2bit(packed, lut)
        out, valid = sq.scan_2bit(packed)
        assert valid.any()
    with Scanner(sm) as sc:
        h, m, bpv = sc._h, packed.shape[0], packed.shape[1]
        o = np.zeros((m, 4))
        with pytest.raises(SgxError, match="Invalid length of dosages"):
            sc.firth_2bit(packed[:, :bpv - 1], lut)
        with pytest.raises(SgxError, match="maxit"):
            sc.firth_2bit(packed, lut, maxit=0)
        for args in ((None, bpv, m, lut.ctypes.data, 50, o.ctypes.data), (packed.ctypes.data, bpv, m, None, 50, o.ctypes.data),
                     (packed.ctypes.data, bpv, m, lut.ctypes.data, 50, None)):
            assert L.sgx_firth_2bit(h, *args) == -1
        assert L.sgx_firth_2bit(h, None, bpv, 0, None, 50, None) == 0                 # no rows: nothing to do
        assert L.sgx_firth_2bit(None, packed.ctypes.data, bpv, m, lut.ctypes.data, 50, o.ctypes.data) == -1
        # the device entry: NULL, stride, alignment
        import torch
        stride = sc.row_stride()
        rows = torch.zeros((m, stride), dtype=torch.uint8, device="cuda")
        tl, od = torch.from_numpy(lut).cuda(), torch.zeros((m, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ok = (rows.data_ptr(), stride, m, tl.data_ptr(), 50, od.data_ptr())
        for i, val in ((0, None), (3, None), (5, None), (1, stride - 64), (1, stride + 16), (0, rows.data_ptr() + 4), (4, 0)):
            args = list(ok)
            args[i] = val
            assert L.sgx_firth_2bit_dev(h, *args) == -1, (i, val)
        assert L.sgx_firth_2bit_dev(h, None, stride, 0, None, 50, None) == 0
        check(sc.firth_2bit(packed, lut), ref, "after the refusals")
        out, valid = sc.scan_2bit(packed)                                             # the handle still scans
        assert valid.shape == (m,) and np.isfinite(out[valid != 0, 5]).all()


def test_memory_returns():
    from saigegds_amd._lib import Scanner, live_bytes
    start = live_bytes()
    sm, packed, lut, _ = _case(50_000)
    sc = Scanner(sm)
    before = live_bytes()
    sc.firth_2bit(packed[:2], lut[:2])
    assert live_bytes() > before                              # the scratch of the long lists, allocated on first use
    held = live_bytes()
    sc.firth_2bit(packed[:2], lut[:2])
    assert live_bytes() == held
    sc.close()
    assert live_bytes() == start


def test_host_rows_in_chunks():
    """sgx_firth_2bit sends its rows up in chunks of pipe_mb MiB at the device stride sgx_row_stride(N) = 128 ceil(N / 512):
    17 536 bytes at N = 70 001, so pipe_mb = 1 is 59 rows a chunk.  60 rows (a chunk and one row) and 125 (two chunks and
    a tail of 7, not a multiple of 16) give the bits of the one-chunk call."""
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 70001, 125
    sm = _model(n)
    rng = np.random.default_rng(12)
    f = rng.choice([0.003, 0.02, 0.1], m)[:, None]
    u = rng.random((m, n))
    codes = ((u < f * f).astype(np.uint8) + (u < 1 - (1 - f) ** 2)).astype(np.uint8)
    codes[rng.random((m, n)) < 0.01] = 3
    packed, lut = pack_dosage_2bit(codes), _tables(codes)
    with Scanner(sm) as sc:
        assert (1 << 20) // sc.row_stride() == 59
        try:
            for rows in (60, m):
                sc.set_option("pipe_mb", 0)
                one = sc.firth_2bit(packed[:rows], lut[:rows])
                sc.set_option("pipe_mb", 1)
                cut = sc.firth_2bit(packed[:rows], lut[:rows])
                assert (one[:, 3] == 1).sum() > rows // 2
                assert one.tobytes() == cut.tobytes(), rows
        finally:
            sc.set_option("pipe_mb", 0)
