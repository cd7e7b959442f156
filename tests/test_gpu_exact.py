"""sgx_exact_2bit(_dev) on the device (kern_exact.h) against the rational reference of tests/exact_ref.py at the parity
rule of DESIGN.md 9 (1e-10 relative on both p-values; MAC and done exact), the tie rule exactly, the rows without a
result, determinism bit for bit, the error paths and the handle's memory.

The bound is not measured but derived: every term of the recurrence and of the tail sums is positive, a carrier costs
at most 3 roundings per entry and a tail sum at most 64, about 260 eps = 6e-14 at MAC 63.  Models: an intercept-only
model written down for every N, its fitted means and trait replaced by those of tests/exact_cases.py (mu in [1e-3,
0.999])."""
from dataclasses import replace

import numpy as np
import pytest

import exact_cases as CS
import exact_ref as R

pytestmark = pytest.mark.gpu
_models = {}


def _model(n, mu=None, y=None):
    from saigegds_amd.nullmod import NullModel, init_nullmod
    if mu is None:
        mu, y = CS.model_values(n)
    X, V = np.ones((n, 1)), mu * (1 - mu)
    mod = NullModel(trait_type="binary", tau=np.array([1.0, 0.0]), fitted_values=mu, sample_id=[f"s{i}" for i in range(n)],
                    var_ratio=np.array([0.94]), y=y, V=V, X1=X, XV=(X * V[:, None]).T, XXVX_inv=X / V.sum())
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, 0.94)
    return replace(sm, mu=mu, y=y, y_mu=y - mu, mu2=mu * (1 - mu))


def _case(n):
    """Per N, made once: the model and the packed rows of the case table."""
    from saigegds_amd.gds import pack_dosage_2bit
    mu, y, codes, lut, ref, _ = CS.case(n)
    if n not in _models:
        _models[n] = (_model(n, mu, y), pack_dosage_2bit(codes))
    return _models[n] + (lut, ref)


def check(out4, ref, what):
    """1e-10 relative on p.mid and p.full, the NaN pattern, MAC and done exact."""
    from conftest import REL_TOL
    assert out4.shape == ref.shape, what
    worst = 0.0
    for c, name in ((0, "p.mid"), (1, "p.full")):
        assert np.array_equal(np.isnan(out4[:, c]), np.isnan(ref[:, c])), f"{what}: NaN pattern of {name}: {out4[:, c]} / {ref[:, c]}"
        ok = ~np.isnan(ref[:, c])
        err = np.abs(out4[ok, c] - ref[ok, c]) / np.abs(ref[ok, c])
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert np.all(err <= REL_TOL), f"{what}: {name} {err}"
    print(f"{what}: off by {worst:.3g} relative at worst ({worst / 2.0 ** -52:.1f} eps)")
    assert np.array_equal(out4[:, 2:], ref[:, 2:]), f"{what}: MAC / done {out4[:, 2:]} / {ref[:, 2:]}"


def _dev_call(sc, packed, lut, max_mac, extra=0, fill=0):
    """The rows through sgx_exact_2bit_dev at the device stride (+ extra bytes of `fill`), bytes beyond the host row `fill` too."""
    import torch
    m, stride = packed.shape[0], sc.row_stride() + extra
    rows = torch.full((m, stride), fill, dtype=torch.uint8)
    rows[:, :packed.shape[1]] = torch.from_numpy(np.ascontiguousarray(packed))
    rows, tl = rows.cuda(), torch.from_numpy(np.ascontiguousarray(lut)).cuda()
    o = torch.full((m, 4), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sc.exact_2bit_dev(rows.data_ptr(), stride, m, tl.data_ptr(), o.data_ptr(), max_mac)
    sc.sync()
    return o.cpu().numpy()


def _beyond_n(packed, n, fill):
    """The codes beyond sample N - 1 in the row's last byte set to those of `fill`."""
    packed = packed.copy()
    if n % 4:
        keep = np.uint8((1 << (2 * (n % 4))) - 1)
        packed[:, -1] = (packed[:, -1] & keep) | (np.uint8(fill) & ~keep)
    return packed


@pytest.mark.parametrize("n", CS.NS)
def test_rows_against_the_reference(n):
    from saigegds_amd._lib import Scanner
    sm, packed, lut, ref = _case(n)
    assert packed.shape[1] == (n + 3) // 4
    with Scanner(sm) as sc:
        check(sc.exact_2bit(packed, lut, 63), ref, f"N={n} host stride ceil(N/4)")
        check(_dev_call(sc, packed, lut, 63), ref, f"N={n} device stride")
        for fill in (0x55, 0xFF):                  # hets / missing codes beyond sample N - 1 and in the padding: none counts
            wide = np.concatenate([_beyond_n(packed, n, fill), np.full((packed.shape[0], 5), fill, dtype=np.uint8)], axis=1)
            check(sc.exact_2bit(wide, lut, 63), ref, f"N={n} host stride + 5, padding {fill:#x}")
            check(_dev_call(sc, _beyond_n(packed, n, fill), lut, 63, extra=64, fill=fill), ref, f"N={n} device stride + 64, padding {fill:#x}")


def test_exact_ties():
    """mu = 0.5 everywhere: two hets, A_obs = 0, no missing -> p.full = 0.5 and p.mid = 0.25 exactly; a het and a hom
    with A_obs = 2 (m' = 1.5, a = 1 ties) -> 1 and 0.75; the same with a missing case (delta = 0.25 (1 - 0.5): m' = 1.375, no
    tie left but a = A_obs itself: d_obs = 0.625, a = 0 and a = 3 beyond) -> p.full = 0.75 and p.mid = 0.625."""
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n = 70
    mu, y = np.full(n, 0.5), np.zeros(n)
    y[[40, 41]] = 1
    codes = np.zeros((3, n), dtype=np.uint8)
    codes[0, [3, 66]] = 1
    codes[1:, 3], codes[1:, 40] = 1, 2
    codes[2, 41] = 3
    lut = np.array([[0, 1, 2, 0.1], [0, 1, 2, 0.1], [0, 1, 2, 0.25]])
    ref = R.exact_ref(mu, y, pack_dosage_2bit(codes), lut, 63)
    assert np.array_equal(ref, [[0.25, 0.5, 2, 1], [0.75, 1, 3, 1], [0.625, 0.75, 3, 1]])
    with Scanner(_model(n, mu, y)) as sc:
        assert np.array_equal(sc.exact_2bit(pack_dosage_2bit(codes), lut, 63), ref)


def test_rows_without_a_result_leave_their_neighbours_alone():
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n = 257
    sm, packed, lut, ref = _case(n)
    mu, y = np.asarray(sm.mu), np.asarray(sm.y)
    good = [0, 2, 6, 9]                                       # MAC 1, 63, a flipped row, 5 % missing
    bad = np.zeros((6, n), dtype=np.uint8)
    bad[0, 5:69] = 1                                          # MAC 64
    bad[1, 10:16] = 1                                         # MAC 6 (> max_mac = 5 below)
    # [2] no carrier
    bad[3:, 100:103] = 1                                      # good rows with bad tables
    bad_lut = CS.tables(bad[[0, 1, 1, 3, 4, 5]])              # ([2]: any valid table)
    bad_lut[3, 1], bad_lut[4, 3], bad_lut[5] = 0.9, np.nan, 0.0
    order = [("g", 0), ("b", 0), ("g", 1), ("b", 2), ("b", 3), ("g", 2), ("b", 4), ("b", 5), ("g", 3)]
    rows = np.concatenate([packed[good[i]:good[i] + 1] if k == "g" else pack_dosage_2bit(bad[i:i + 1]) for k, i in order])
    tabs = np.array([lut[good[i]] if k == "g" else bad_lut[i] for k, i in order])
    is_good = np.array([k == "g" for k, _ in order])
    want = R.exact_ref(mu, y, rows, tabs, 63)
    assert np.array_equal(want[is_good], ref[good]) and not want[~is_good, 3].any()
    assert list(want[~is_good, 2]) == [64, 0, 0, 0, 0]
    with Scanner(sm) as sc:
        alone = sc.exact_2bit(packed[good], lut[good], 63)
        got = sc.exact_2bit(rows, tabs, 63)
        check(got, want, "bad rows between good ones")
        assert np.array_equal(got[is_good], alone)              # bit for bit what the good rows give on their own
        # max_mac + 1: the MAC 6 row at max_mac = 5 (and the good rows above 5 with it), done at max_mac = 6
        mac6 = pack_dosage_2bit(bad[1:2])
        three = np.concatenate([packed[0:1], mac6, packed[1:2]])
        t3 = np.array([lut[0], bad_lut[1], lut[1]])
        at5, at6 = sc.exact_2bit(three, t3, 5), sc.exact_2bit(three, t3, 6)
        check(at5, R.exact_ref(mu, y, three, t3, 5), "max_mac = 5")
        check(at6, R.exact_ref(mu, y, three, t3, 6), "max_mac = 6")
        assert list(at5[:, 3]) == [1, 0, 1] and list(at6[:, 3]) == [1, 1, 1] and at5[1, 2] == 6
        assert np.array_equal(at5[[0, 2]], at6[[0, 2]])


@pytest.fixture(scope="module")
def many():
    """5 000 rows at N = 257 (more than any grid holds in one round): MAC from 0 to beyond 63, both orientations, 1 % missing."""
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 257, 5000
    rng = np.random.default_rng(17)
    f = rng.choice([0.002, 0.01, 0.03, 0.15, 0.97], m, p=[0.3, 0.3, 0.2, 0.1, 0.1])[:, None]
    u = rng.random((m, n))
    codes = ((u < f * f).astype(np.uint8) + (u < 1 - (1 - f) ** 2)).astype(np.uint8)
    codes[rng.random((m, n)) < 0.01] = 3
    return _case(n)[0], pack_dosage_2bit(codes), CS.tables(codes)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_bits_do_not_depend_on_position_order_call_or_chunk(many):
    """The same rows permuted, repeated, in a second call, through the device entry, and through the host entry in
    several chunks: sgx_exact_2bit sends its rows up in chunks of pipe_mb MiB at the device stride (128 bytes at N =
    257), so pipe_mb = 1 is 8192 rows a chunk -- the 5 000 rows twice over are a chunk and a tail of 1808."""
    from saigegds_amd._lib import Scanner
    sm, packed, lut = many
    m = packed.shape[0]
    with Scanner(sm) as sc:
        full = sc.exact_2bit(packed, lut, 63)
        assert _same(full, sc.exact_2bit(packed, lut, 63))                              # a second call
        perm = np.random.default_rng(5).permutation(m)
        assert _same(full[perm], sc.exact_2bit(packed[perm], lut[perm], 63))            # permuted
        for j in (0, 1, 3, 4, 2047, 2048, m - 1):                                       # a row alone
            assert _same(sc.exact_2bit(packed[j:j + 1], lut[j:j + 1], 63)[0], full[j]), j
        assert _same(_dev_call(sc, packed, lut, 63), full)                              # the device entry
        twice, lut2 = np.concatenate([packed, packed[::-1]]), np.concatenate([lut, lut[::-1]])
        assert (1 << 20) // sc.row_stride() == 8192 < 2 * m
        try:
            sc.set_option("pipe_mb", 0)
            one = sc.exact_2bit(twice, lut2, 63)
            sc.set_option("pipe_mb", 1)
            cut = sc.exact_2bit(twice, lut2, 63)
        finally:
            sc.set_option("pipe_mb", 0)
        assert _same(one, cut) and _same(one, np.concatenate([full, full[::-1]]))       # repeated, in chunks
    done = full[:, 3] == 1
    print(f"{int(done.sum())} of {m} rows done, MAC up to {int(full[:, 2].max())}")
    assert 0.5 * m < done.sum() < m and (full[:, 2] == 0).any() and (full[:, 2] > 63).any()
    assert np.all((full[done, 0] > 0) & (full[done, 0] <= full[done, 1]) & (full[done, 1] <= 1 + 1e-12))
    assert np.isnan(full[~done, :2]).all()
    sample = np.flatnonzero(done)[::97]                                                 # and they are the right bits
    check(full[sample], R.exact_ref(sm.mu, sm.y, packed[sample], lut[sample], 63), "a sample of the 5 000 rows")


def test_refusals_leave_the_handle_usable():
    import torch
    from saigegds_amd._lib import Scanner, SgxError, load
    from test_gpu_skat import _model as skat_model
    sm, packed, lut, ref = _case(1000)
    L = load()
    with Scanner(skat_model(1000, "quantitative")) as sq:
        with pytest.raises(SgxError, match="binary"):
            sq.exact_2bit(packed, lut, 10)
        out, valid = sq.scan_2bit(packed)
        assert valid.shape == (packed.shape[0],)
    with Scanner(sm) as sc:
        h, m, bpv = sc._h, packed.shape[0], packed.shape[1]
        o = np.zeros((m, 4))
        with pytest.raises(SgxError, match="Invalid length of dosages"):
            sc.exact_2bit(packed[:, :bpv - 1], lut, 10)
        for bad in (0, 64, -1):
            with pytest.raises(SgxError, match="max_mac"):
                sc.exact_2bit(packed, lut, bad)
        for args in ((None, bpv, m, lut.ctypes.data, 10, o.ctypes.data), (packed.ctypes.data, bpv, m, None, 10, o.ctypes.data),
                     (packed.ctypes.data, bpv, m, lut.ctypes.data, 10, None)):
            assert L.sgx_exact_2bit(h, *args) == -1
        assert L.sgx_exact_2bit(h, None, bpv, 0, None, 10, None) == 0                 # no rows: nothing to do
        assert L.sgx_exact_2bit(None, packed.ctypes.data, bpv, m, lut.ctypes.data, 10, o.ctypes.data) == -1
        assert not o.any()
        # the device entry: NULL, max_mac, stride, alignment
        stride = sc.row_stride()
        rows = torch.zeros((m, stride), dtype=torch.uint8, device="cuda")
        tl, od = torch.from_numpy(lut).cuda(), torch.zeros((m, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ok = (rows.data_ptr(), stride, m, tl.data_ptr(), 10, od.data_ptr())
        for i, val in ((0, None), (3, None), (5, None), (1, stride - 64), (1, stride + 16), (0, rows.data_ptr() + 4),
                       (3, tl.data_ptr() + 4), (4, 0), (4, 64)):
            args = list(ok)
            args[i] = val
            assert L.sgx_exact_2bit_dev(h, *args) == -1, (i, val)
        assert L.sgx_exact_2bit_dev(h, None, stride, 0, None, 10, None) == 0
        sc.sync()
        assert not od.cpu().numpy().any()                                             # nothing was launched
        check(sc.exact_2bit(packed, lut, 63), ref, "after the refusals")
        out, valid = sc.scan_2bit(packed)                                             # the handle still scans
        assert valid.shape == (m,)


def test_memory_returns():
    from saigegds_amd._lib import Scanner, live_bytes
    start = live_bytes()
    sm, packed, lut, _ = _case(4097)
    sc = Scanner(sm)
    sc.exact_2bit(packed[:2], lut[:2], 63)
    held = live_bytes()
    assert held > start
    sc.exact_2bit(packed[:2], lut[:2], 63)
    assert live_bytes() == held                               # no scratch: nothing but the staging buffer of the first call
    sc.close()
    assert live_bytes() == start
