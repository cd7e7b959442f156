"""The reference of the Firth effect sizes (tests/firth_ref.py) against closed forms and against its own definition
evaluated in mpmath.  No GPU."""
import numpy as np
import pytest

import firth_ref as R

LD = np.longdouble


def _logit(p):
    return np.log(p / (1 - p))


@pytest.mark.parametrize("y", [0, 1])
@pytest.mark.parametrize("g", [1.0, 2.0, 0.37])
@pytest.mark.parametrize("mu", [0.3, 1e-4])
def test_one_carrier(y, g, mu):
    """One entry: U* = g (y - p) + g (1 - 2p) / 2 = 0 at p = (y + 1/2) / 2, where w = 3/16."""
    beta, se = R.firth_list([g], [mu], [y])
    p = (LD(y) + LD(0.5)) / 2
    want = (_logit(p) - _logit(LD(mu))) / LD(g)
    assert abs(beta - want) <= 4e-16 * max(1, abs(want)), (beta, want)
    assert abs(se - 1 / (LD(g) * np.sqrt(LD(3) / 16))) <= 1e-15 * se


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_equal_carriers_all_cases(n):
    """n entries of one mu and g = 1, all cases: n (1 - p) + (1 - 2p) / 2 = 0 at p = (n + 1/2) / (n + 1)."""
    mu = 0.02
    beta, se = R.firth_list(np.ones(n), np.full(n, mu), np.ones(n))
    p = (LD(n) + LD(0.5)) / (n + 1)
    want = _logit(p) - _logit(LD(mu))
    assert abs(beta - want) <= 4e-16 * abs(want)
    assert abs(se - 1 / np.sqrt(n * p * (1 - p))) <= 1e-15 * se


def test_no_information():
    assert all(np.isnan(v) for v in R.firth_list([], [], []))


def _random_row(rng):
    n = int(rng.integers(2, 400))
    g = rng.choice([1.0, 2.0, float(rng.uniform(0.01, 0.6))], size=n, p=[0.8, 0.15, 0.05])
    mu = rng.uniform(0.001, 0.5, n)
    y = (rng.random(n) < np.minimum(0.9, 3 * mu)).astype(np.float64)          # carriers enriched among the cases
    return g, mu, y


def test_root_of_the_definition_in_mpmath():
    """Twenty random rows.  U* of the definition, written out in mpmath at 50 digits, has a root at which it is 0 to
    1e-25, and the reference's long-double root is that root: a long double cannot itself make U* smaller than
    |dU*/dbeta| times its own spacing (1e-19 |beta|), so the 1e-25 is asked of the root polished in mpmath from the
    reference's, and the reference has to lie within 1e-15 max(1, |beta|) of it -- its bisection stops at a bracket of
    1e-16 max(1, |beta|), and where the long-double U* is below its own rounding error (400 terms of size <= 2 at
    2^-64: 4e-17, over |dU*/dbeta| >= 0.1 on these rows) it can take the wrong side."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(20261020)
    worst = 0.0
    for _ in range(20):
        g, mu, y = _random_row(rng)
        beta, se = R.firth_list(g, mu, y)
        G, M = [mp.mpf(float(v)) for v in g], [mp.mpf(float(v)) for v in mu]

        def parts(b):
            i = a = u = mp.mpf(0)
            for gi, mi, yi in zip(G, M, y):
                p = 1 / (1 + mp.exp(-(mp.log(mi / (1 - mi)) + b * gi)))
                w = p * (1 - p)
                i += w * gi ** 2
                a += w * (1 - 2 * p) * gi ** 3
                u += gi * (yi - p)
            return i, a, u

        def ustar(b):
            i, a, u = parts(b)
            return u + a / (2 * i)

        b0 = mp.mpf(float(beta)) + mp.mpf(float(beta - LD(float(beta))))
        root = mp.findroot(ustar, b0, tol=1e-40)
        assert abs(ustar(root)) <= mp.mpf("1e-25")
        err = float(abs(root - b0) / max(1, abs(root)))
        worst = max(worst, err)
        assert err <= 1e-15, (err, float(root))
        assert abs(float(se) * float(mp.sqrt(parts(root)[0])) - 1) <= 1e-14
    print(f"long-double root against the mpmath root: {worst:.3g} relative at worst")


def test_newton_restatement_meets_the_reference():
    """The kernel's iteration in float64 (firth_ref.newton_f64) converges on the rows above and on the hard ones --
    one carrier, all carriers cases at mu = 1e-4 -- to the reference's root."""
    rng = np.random.default_rng(5)
    rows = [_random_row(rng) for _ in range(20)]
    rows.append(([1.0], [0.01], [1.0]))
    rows.append((np.ones(5), np.full(5, 1e-4), np.ones(5)))
    rows.append((np.ones(40), rng.uniform(0.01, 0.3, 40), np.zeros(40)))
    worst = 0.0
    for g, mu, y in rows:
        beta, se = R.firth_list(g, mu, y)
        b, s, it, ok = R.newton_f64(g, mu, y)
        assert ok and it <= 50
        worst = max(worst, abs(b - float(beta)) / max(1e-300, abs(float(beta))), abs(s - float(se)) / float(se))
    print(f"float64 iteration against the reference: {worst:.3g} relative at worst")
    assert worst <= 1e-10
