"""Reference of the exact p-values (sgx_exact_2bit, saigegds_amd.exact) -- TEST INFRASTRUCTURE ONLY.

A restatement of the DEFINITION in exact rational arithmetic (``fractions.Fraction`` of the doubles, ``delta`` and
``m'`` included), sharing nothing with the kernel: up to ``ENUM_MAX`` carriers every one of the ``2^c`` phenotype
configurations is listed with its probability and its ``A``; above that the pmf comes from the recurrence, in
``Fraction`` too.  ``RefScanner`` puts it (with the CPU scan oracle and the Firth reference) behind the interface of
``saigegds_amd._lib.Scanner`` that the single-variant driver and ``exact_pass`` use, so that they run without a GPU."""
from fractions import Fraction

import numpy as np

import firth_ref

ENUM_MAX = 12
NOT_DONE = (np.nan, np.nan, 0.0, 0.0)


def table_ok(t):
    return bool(t[1] == 1 and ((t[0] == 0 and t[2] == 2) or (t[0] == 2 and t[2] == 0)) and np.isfinite(t[3]))


def row_parts(codes, t, mu, y):
    """One row by the definition -> (g, mu, y of the carriers in sample order as int / Fraction / int, m' as a Fraction)."""
    t = [float(v) for v in t]
    g_all = np.array([t[0], t[1], t[2], 0.0])[codes]
    car = np.flatnonzero((codes < 3) & ((g_all == 1) | (g_all == 2)))
    mis = np.flatnonzero(codes == 3)
    delta = Fraction(t[3]) * sum((Fraction(float(y[i])) - Fraction(float(mu[i])) for i in mis), Fraction(0))
    g = [int(g_all[i]) for i in car]
    fm = [Fraction(float(mu[i])) for i in car]
    yy = [int(y[i] != 0) for i in car]
    mp = sum((gi * mi for gi, mi in zip(g, fm)), Fraction(0)) - delta
    return g, fm, yy, mp


def pmf_enumerated(g, fm):
    """f by listing all 2^c configurations: every configuration's probability lands on its A."""
    conf = [(Fraction(1), 0)]
    for gi, mi in zip(g, fm):                                   # every configuration splits in two: y_i = 0, y_i = 1
        conf = [c for pr, a in conf for c in ((pr * (1 - mi), a), (pr * mi, a + gi))]
    assert len(conf) == 2 ** len(g)
    f = [Fraction(0)] * (sum(g) + 1)
    for pr, a in conf:
        f[a] += pr
    return f


def pmf_recurrence(g, fm):
    """f by the recurrence f[a] <- (1 - mu) f[a] + mu f[a - g]."""
    f = [Fraction(1)] + [Fraction(0)] * sum(g)
    for gi, mi in zip(g, fm):
        f = [(1 - mi) * f[a] + (mi * f[a - gi] if a >= gi else 0) for a in range(len(f))]
    return f


def tails(f, mp, a_obs):
    """(p.mid, p.full, smallest non-zero |d_a - d_obs| over a != A_obs) in rationals."""
    d_obs = abs(a_obs - mp)
    gt = sum((fa for a, fa in enumerate(f) if abs(a - mp) > d_obs), Fraction(0))
    eq = sum((fa for a, fa in enumerate(f) if abs(a - mp) == d_obs), Fraction(0))
    gaps = [abs(abs(a - mp) - d_obs) for a in range(len(f)) if a != a_obs]
    gaps = [x for x in gaps if x != 0]
    return gt + eq / 2, gt + eq, (min(gaps) if gaps else None)


def exact_row(codes, t, mu, y, max_mac, with_gap=False):
    """out4 of one row: (p.mid, p.full, MAC, done) as floats; with_gap: the smallest non-zero gap (a Fraction or None) too."""
    if not table_ok(t):
        return NOT_DONE + ((None,) if with_gap else ())
    g, fm, yy, mp = row_parts(codes, t, mu, y)
    mac = sum(g)
    if mac == 0 or mac > max_mac:
        return (np.nan, np.nan, float(mac), 0.0) + ((None,) if with_gap else ())
    f = pmf_enumerated(g, fm) if len(g) <= ENUM_MAX else pmf_recurrence(g, fm)
    assert sum(f) == 1
    mid, full, gap = tails(f, mp, sum(gi * yi for gi, yi in zip(g, yy)))
    return (float(mid), float(full), float(mac), 1.0) + ((gap,) if with_gap else ())


def exact_ref(mu, y, packed, lut, max_mac, n=None):
    """What ``Scanner.exact_2bit`` returns, by the definition: out4 [m, 4] float64."""
    from saigegds_amd.gds import unpack_dosage_2bit
    mu, y = np.asarray(mu, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 4)
    codes = unpack_dosage_2bit(np.asarray(packed), mu.size if n is None else n)
    return np.array([exact_row(codes[j], lut[j], mu, y, max_mac) for j in range(lut.shape[0])]).reshape(-1, 4)


class RefScanner(firth_ref.RefScanner):
    """The CPU scan oracle, ``firth_ref`` and ``exact_ref`` behind the part of ``Scanner`` the single-variant driver uses."""

    exact_calls = []     # (mu of the model, number of rows, max_mac) of every exact_2bit call, for the tests

    def scan_u8(self, dosage):
        return self._o.scan_u8(dosage)

    def scan_f64(self, dosage):
        return self._o.scan_f64(dosage)

    def exact_2bit(self, packed, lut, max_mac):
        RefScanner.exact_calls.append((np.asarray(self.sm.mu).copy(), np.asarray(packed).shape[0], int(max_mac)))
        return exact_ref(self.sm.mu, self.sm.y, packed, lut, max_mac)
