"""Reference of the Firth effect sizes (sgx_firth_2bit, saigegds_amd.firth) -- TEST INFRASTRUCTURE ONLY.

A long-double restatement of the DEFINITION, independent of the kernel's iteration and of its arithmetic: p from the
logistic function of ``logit mu + beta g``, the root of U* by a sign bracket and plain bisection to 1e-16.  ``RefScanner``
puts it (and the CPU scan oracle) behind the interface of ``saigegds_amd._lib.Scanner`` that the single-variant driver
and ``firth_pass`` use, so that they run without a GPU.  ``newton_f64`` restates the kernel's iteration in float64
numpy: what the kernel's trajectory costs against this reference is measured with it, on the CPU."""
import numpy as np

LD = np.longdouble


def _pq(beta, g, mu):
    eta = np.log(mu / (1 - mu)) + beta * g
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-eta)), 1 / (1 + np.exp(eta))


def sums(beta, g, mu, y):
    """(I, A, B, sum g (y - p)) at beta over a list (long double)."""
    p, q = _pq(LD(beta), g, mu)
    w = p * q
    return (np.sum(w * g ** 2), np.sum(w * (q - p) * g ** 3), np.sum(w * (1 - 6 * w) * g ** 4),
            np.sum(g * np.where(y != 0, q, -p)))


def ustar(beta, g, mu, y):
    i, a, _, u = sums(beta, g, mu, y)
    return u + a / (2 * i)


def firth_list(g, mu, y):
    """The root of U* and 1 / sqrt(I) there for one list of (g != 0, mu, y) -> (beta, SE) as long doubles; (NaN, NaN)
    where there is no information (no entry, I = 0)."""
    g, mu, y = (np.asarray(a, dtype=LD) for a in (g, mu, y))
    if g.size == 0 or not sums(0, g, mu, y)[0] > 0:
        return LD("nan"), LD("nan")
    lo, hi = LD(-1), LD(1)
    while not ustar(lo, g, mu, y) > 0:        # U* -> sum g y + |g| / 2 > 0 towards -inf, -> < 0 towards +inf
        lo *= 2
        assert lo > -4096
    while not ustar(hi, g, mu, y) < 0:
        hi *= 2
        assert hi < 4096
    while hi - lo > LD(1e-16) * max(LD(1), abs(lo), abs(hi)):
        mid = (lo + hi) / 2
        if mid == lo or mid == hi:
            break
        if ustar(mid, g, mu, y) > 0:
            lo = mid
        else:
            hi = mid
    beta = (lo + hi) / 2
    return beta, 1 / np.sqrt(sums(beta, g, mu, y)[0])


def row_lists(packed, lut, mu, y):
    """Per row the list the kernel builds: (g, mu, y) of the samples with g != 0, ascending."""
    from saigegds_amd.gds import unpack_dosage_2bit
    codes = unpack_dosage_2bit(packed, mu.size)
    for j in range(codes.shape[0]):
        g = np.asarray(lut[j], dtype=np.float64)[codes[j]]
        keep = g != 0
        yield g[keep], mu[keep], y[keep]


def firth_ref(sm, packed, lut):
    """What ``Scanner.firth_2bit`` returns, by the definition: out4 [m, 4] float64 = beta, SE, NaN (the iterations are
    the kernel's own), converged."""
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 4)
    mu, y = np.asarray(sm.mu, dtype=np.float64), np.asarray(sm.y, dtype=np.float64)
    out = np.full((lut.shape[0], 4), np.nan)
    out[:, 3] = 0
    for j, (g, m, yy) in enumerate(row_lists(packed, lut, mu, y)):
        if not np.all(np.isfinite(lut[j])):
            continue
        b, se = firth_list(g, m, yy)
        if np.isfinite(b):
            out[j] = float(b), float(se), np.nan, 1.0
    return out


def newton_f64(g, mu, y, maxit=50):
    """The kernel's iteration in float64 numpy (kern_firth.h, phase B) -> (beta, SE, iterations, converged)."""
    g, mu, y = (np.asarray(a, dtype=np.float64) for a in (g, mu, y))

    def s4(b):
        x = b * g
        with np.errstate(over="ignore"):
            a = mu * np.where(x <= 0, np.exp(np.minimum(x, 0)), 1.0)
            c = (1 - mu) * np.where(x <= 0, 1.0, np.exp(-np.maximum(x, 0)))
        p, q = a / (a + c), c / (a + c)
        w = p * q
        return (np.sum(w * g * g), np.sum(w * (q - p) * g ** 3), np.sum(w * (1 - 6 * w) * g ** 4),
                np.sum(g * np.where(y != 0, q, -p)))
    beta, lo, hi = 0.0, -np.inf, np.inf
    if g.size == 0:
        return np.nan, np.nan, 0, False
    for it in range(1, maxit + 1):
        i, a, bb, u = s4(beta)
        if not i > 0:
            return np.nan, np.nan, it, False
        u = u + 0.5 * a / i
        du = -i + 0.5 * (bb / i - (a / i) ** 2)
        if u > 0:
            lo = beta
        elif u < 0:
            hi = beta
        d = -u / du if du < 0 else u / i
        d = min(5.0, max(-5.0, d))
        nb = beta + d
        if np.isfinite(lo) and np.isfinite(hi) and nb != beta and not lo < nb < hi:
            nb = 0.5 * (lo + hi)
        if u == 0:
            nb = beta
        d, beta = nb - beta, nb
        if abs(d) <= 1e-12 * max(1.0, abs(beta)):
            return beta, 1 / np.sqrt(s4(beta)[0]), it, True
    return beta, np.nan, maxit, False


class RefScanner:
    """The CPU scan oracle and ``firth_ref`` behind the part of ``Scanner`` the single-variant driver uses."""

    calls = []           # (mu of the model, number of rows) of every firth_2bit call, for the tests

    def __init__(self, sm, device=0):
        from oracle import Oracle
        self.sm, self._o = sm, Oracle(sm)

    def scan_2bit(self, packed):
        return self._o.scan_2bit(packed)

    def firth_2bit(self, packed, lut, maxit=50):
        RefScanner.calls.append((np.asarray(self.sm.mu).copy(), np.asarray(packed).shape[0]))
        return firth_ref(self.sm, packed, lut)

    def close(self):
        self._o.close()
