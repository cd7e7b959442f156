"""The LD statistic on the CPU: the conditions on the test inputs under which the double and the exact
decision agree, the constructed tie, and the numpy side of the public surface (``ld_corr``)."""
import numpy as np
import pytest

import ld_cases as LC
import ld_ref as R


def _decided_inputs():
    """Every table of rows on which a test takes an in-LD decision against the reference, with the t2 it takes it at
    (the constructed tie apart: it sits on the threshold on purpose and has its own test)."""
    for name in ("DRIVER_CPU", "DRIVER_GPU", "FLAG_ROWS"):
        codes = LC.ld_source(**getattr(LC, name))[0]
        yield name, codes, [t * t for t in LC.THRESHOLDS]
        if name in LC.SUBSETS:
            yield name + " subset", codes[:, LC.subset(name, codes.shape[1])], [t * t for t in LC.THRESHOLDS]
    yield "RING", LC.ring_codes(), [LC.RING["t2"]]


INPUTS = ["DRIVER_CPU", "DRIVER_CPU subset", "DRIVER_GPU", "DRIVER_GPU subset", "FLAG_ROWS", "RING"]


@pytest.mark.parametrize("name", INPUTS)
def test_no_test_input_sits_at_a_threshold(name):
    """No pair with vx, vy > 0 has c^2 / (vx vy) within a relative 1e-9 of t2, for every t2 the tests decide at on that
    input: then the double decision (three roundings, each 2^-53) equals the exact one.  A condition on the inputs, not
    a tolerance."""
    assert [k for k, _, _ in _decided_inputs()] == INPUTS
    codes, t2s = next((c, t) for k, c, t in _decided_inputs() if k == name)
    s = R.counts(codes, codes)
    for t2 in t2s:
        gap = R.min_rel_gap(s, t2)
        assert gap > 1e-9, (name, t2, gap)


def test_double_and_exact_decisions_agree_on_the_inputs():
    codes = LC.ld_source(**LC.DRIVER_CPU)[0]
    s = R.counts(codes, codes)
    for t in LC.THRESHOLDS:
        assert np.array_equal(R.in_ld(s, t * t), R.in_ld_exact(s, t * t))
    for n, ma, mb in LC.COUNT_CASES[:8]:
        c = LC.random_codes(n, ma + mb, 100 + n)
        s = R.counts(c[:ma], c[ma:])
        assert R.min_rel_gap(s, 0.04) > 1e-9
        assert np.array_equal(R.in_ld(s, 0.04), R.in_ld_exact(s, 0.04))


def test_constructed_tie():
    """x = (0,1,1,2), y = (0,1,2,1): c = 4, vx = vy = 8, r = 1/2 exactly -- not in LD at t = 0.5 (strict), in LD just
    below it."""
    s = R.counts(np.array([LC.TIE_X]), np.array([LC.TIE_Y]))
    assert s[0, 0].tolist() == [4, 4, 4, 6, 6, 5]
    assert [int(v[0, 0]) for v in R.cvv(s)] == [4, 8, 8]
    lo = float(np.nextafter(0.5, 0))
    for f in (R.in_ld, R.in_ld_exact):
        assert not f(s, 0.5 * 0.5)[0, 0]
        assert f(s, lo * lo)[0, 0]


def test_special_rows_of_the_case_table():
    c = LC.random_codes(65, 8, 3)
    s = R.counts(c, c)
    assert (s[0] == 0).all() and (s[:, 0] == 0).all()            # all missing
    assert R.cvv(s)[1][1, 5] == 0                                 # monomorphic: vx = 0
    assert s[2, 3, 0] == 0 and s[4, 5, 0] == 1                    # disjoint called sets, one common sample
    assert not R.in_ld(s, 0.0)[[0, 1, 2, 4], [5, 5, 3, 5]].any()


def test_ld_corr():
    from saigegds_amd import ld_corr
    codes = LC.ld_source(**LC.DRIVER_CPU)[0][:40]
    s = R.counts(codes, codes)
    r = ld_corr(s)
    assert r.shape == (40, 40)
    assert np.isnan(r[5]).all() and np.isnan(r[:, 5]).all()       # the monomorphic row
    for i, j in ((0, 1), (3, 2), (20, 21)):
        both = (codes[i] != 3) & (codes[j] != 3)
        want = np.corrcoef(codes[i][both].astype(float), codes[j][both].astype(float))[0, 1]
        assert abs(r[i, j] - want) < 1e-12
    tie = ld_corr(R.counts(np.array([LC.TIE_X]), np.array([LC.TIE_Y])))
    assert tie[0, 0] == 0.5
