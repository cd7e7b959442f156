"""The exact-p-value reference against itself (tests/exact_ref.py) and the case table of the GPU test
(tests/exact_cases.py), on the CPU: enumeration of the 2^c configurations against the rational recurrence, the tie
rule, the rows without a result, and the gap that keeps double and rational comparisons in agreement."""
from fractions import Fraction

import numpy as np
import pytest

import exact_cases as CS
import exact_ref as R


@pytest.mark.parametrize("c", [1, 2, 3, 7, 12])
def test_enumeration_is_the_recurrence(c):
    rng = np.random.default_rng(c)
    for rep in range(3):
        g = [int(v) for v in rng.integers(1, 3, c)]
        fm = [Fraction(float(v)) for v in rng.uniform(1e-3, 0.999, c)]
        fe, fr = R.pmf_enumerated(g, fm), R.pmf_recurrence(g, fm)
        assert fe == fr and sum(fe) == 1 and len(fe) == sum(g) + 1
        mp = Fraction(float(rng.uniform(0, sum(g))))
        for a_obs in (0, sum(g) // 2, sum(g)):
            assert R.tails(fe, mp, a_obs) == R.tails(fr, mp, a_obs)


def test_ties_are_halved():
    """mu = 0.5, two hets, A_obs = 0: f = [1/4, 1/2, 1/4], m' = 1, a = 0 and a = 2 tie."""
    mu, y = np.full(8, 0.5), np.zeros(8)
    codes = np.zeros(8, dtype=np.uint8)
    codes[[2, 5]] = 1
    assert R.exact_row(codes, [0, 1, 2, 0.5], mu, y, 63) == (0.25, 0.5, 2.0, 1.0)
    # a het and a hom at mu = 0.5, the hom a case: f = [1/4] * 4 on a = 0..3, m' = 1.5, A_obs = 2 ties with a = 1
    codes[5], y[5] = 2, 1
    assert R.exact_row(codes, [0, 1, 2, 0.5], mu, y, 63) == (0.75, 1.0, 3.0, 1.0)
    # ... and read the other way round (flipped table, codes swapped): the same test
    assert R.exact_row(np.array([2, 1, 0, 3], dtype=np.uint8)[codes], [2, 1, 0, 0.5], mu, y, 63) == (0.75, 1.0, 3.0, 1.0)


def test_missing_samples_shift_the_centre_only():
    mu, y = np.array([0.25, 0.5, 0.125, 0.5]), np.array([1.0, 0.0, 1.0, 0.0])
    codes = np.array([1, 3, 3, 0], dtype=np.uint8)
    g, fm, yy, mp = R.row_parts(codes, [0, 1, 2, 0.5], mu, y)
    assert (g, fm, yy) == ([1], [Fraction(1, 4)], [1])
    assert mp == Fraction(1, 4) - Fraction(1, 2) * (Fraction(-1, 2) + Fraction(7, 8))
    # m' = 1/16: d_0 = 1/16 < d_obs = 15/16
    assert R.exact_row(codes, [0, 1, 2, 0.5], mu, y, 63) == (0.125, 0.25, 1.0, 1.0)


def test_rows_without_a_result():
    mu, y = np.full(70, 0.3), np.zeros(70)
    codes = np.zeros(70, dtype=np.uint8)
    nan2 = lambda r: np.isnan(r[0]) and np.isnan(r[1])
    r = R.exact_row(codes, [0, 1, 2, 0.1], mu, y, 63)
    assert nan2(r) and r[2:] == (0.0, 0.0)                     # no carrier
    codes[:64] = 1
    r = R.exact_row(codes, [0, 1, 2, 0.1], mu, y, 63)
    assert nan2(r) and r[2:] == (64.0, 0.0)                    # MAC 64
    codes[63] = 0
    assert R.exact_row(codes, [0, 1, 2, 0.1], mu, y, 63)[2:] == (63.0, 1.0)
    assert R.exact_row(codes, [0, 1, 2, 0.1], mu, y, 62)[2:] == (63.0, 0.0)
    for bad in ([0, 0.9, 2, 0.1], [0, 1, 2, np.nan], [0, 0, 0, 0], [0, 1, 2, np.inf], [2, 1, 2, 0.1], [0, 1, 0, 0.1]):
        r = R.exact_row(codes, bad, mu, y, 63)
        assert nan2(r) and r[2:] == (0.0, 0.0), bad


@pytest.mark.parametrize("n", CS.NS)
def test_case_table_keeps_its_distance_from_ties(n):
    """For every a != A_obs the gap |d_a - d_obs| is exactly 0 or at least 1e-6 (in rationals); every row of the table
    has a result at n >= 3, MAC 63 is there from n = 63 on, and the missing rows have a non-zero delta."""
    mu, y, codes, lut, ref, gaps = CS.case(n)
    assert mu.min() >= 1e-3 and mu.max() <= 0.999
    assert codes.shape == (len(CS.ROWS), n) and ref.shape == (len(CS.ROWS), 4)
    for j, gap in enumerate(gaps):
        assert gap is None or gap >= Fraction(1, 10 ** 6), (n, CS.ROWS[j], float(gap))
    if n >= 3:
        assert np.all(ref[:, 3] == 1) and np.all((ref[:, 0] > 0) & (ref[:, 0] <= ref[:, 1]) & (ref[:, 1] <= 1))
        assert lut[6, 0] == 2 and lut[7, 0] == 2 and lut[0, 0] == 0
        for j in (7, 8, 9, 10):
            mis = codes[j] == 3
            assert mis.any() and lut[j, 3] * np.sum(y[mis] - mu[mis]) != 0
        assert (codes[9] == 3).sum() == max(1, n // 20)
    if n >= 63:
        assert ref[2, 2] == 63
    assert ref[0, 2] == 1 and ref[1, 2] == 2
