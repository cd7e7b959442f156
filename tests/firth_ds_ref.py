"""Reference of sgx_ds_block_firth (DosageBlock.firth) -- TEST INFRASTRUCTURE ONLY.

The dosage twin of tests/firth_ref.py: the list of a row is built with numpy from ``(x, flip, mean)`` exactly as the
entry is defined,
    g(i) = present(x) ? (flip ? 2 - x : x) : mean
(uint8: 0xFF missing; int32: NA_INTEGER missing; float64: non-finite missing), the samples with ``g != 0`` in ascending
order, and goes to ``firth_ref.firth_list`` (long double, bracket and bisection: nothing of the kernel's iteration).
``RefDsScanner`` puts it behind the part of ``Scanner`` / ``DosageBlock`` that the single-variant driver and
``firth_pass`` use for dosage input -- a block with ``load``, ``scan`` and ``firth`` -- so that they run without a GPU."""
import numpy as np

import firth_ref as R
from aggregate_ds_ref import as_f64, ok_mask


def ds_values(x, flip, mean):
    """g of one row in float64 (every operation is exact or the single rounding of 2 - x)."""
    x = np.asarray(x)
    ok = ok_mask(x)
    v = np.where(ok, x, 0).astype(np.float64)
    return np.where(ok, 2 - v if flip else v, np.float64(mean))


def ds_list(x, flip, mean, mu, y):
    """The list the kernel builds of one row: (g, mu, y) of the samples with g != 0, ascending."""
    g = ds_values(x, flip, mean)
    keep = g != 0
    return g[keep], np.asarray(mu)[keep], np.asarray(y)[keep]


def firth_ds_ref(sm, rows, flip, mean):
    """What ``DosageBlock.firth`` returns for the rows, one (flip, mean) each, by the definition: out4 [m, 4] float64 =
    beta, SE, NaN (the iterations are the kernel's own), converged.  A non-finite mean: NaN, NaN, NaN, 0."""
    mu, y = np.asarray(sm.mu, dtype=np.float64), np.asarray(sm.y, dtype=np.float64)
    out = np.full((len(rows), 4), np.nan)
    out[:, 3] = 0
    for j, row in enumerate(rows):
        if not np.isfinite(mean[j]):
            continue
        b, se = R.firth_list(*ds_list(row, flip[j], mean[j], mu, y))
        if np.isfinite(b):
            out[j] = float(b), float(se), np.nan, 1.0
    return out


class _RefDsBlock:
    """``load`` / ``scan`` / ``firth`` of a batch of dosage rows: numpy counts, the CPU scan oracle, ``firth_ds_ref``."""

    def __init__(self, sc, dtype, cap):
        self.sc, self.dtype, self.cap, self.rows = sc, np.dtype(dtype), int(cap), None

    def load(self, dosage):
        assert dosage.dtype == self.dtype and dosage.shape[0] <= self.cap and dosage.shape[1] == self.sc.sm.n
        self.rows = dosage.copy()
        ok = np.stack([ok_mask(r) for r in self.rows])
        n = ok.sum(axis=1).astype(np.int32)
        if self.dtype == np.float64:
            z = np.where(ok, self.rows, 0.0)
            return n, z.sum(axis=1), np.floor(z).astype(np.int64).sum(axis=1)
        z = np.where(ok, self.rows, 0).astype(np.int64).sum(axis=1)
        return n, z.astype(np.float64), z

    def scan(self):
        return self.sc.scan_f64(np.stack([as_f64(r) for r in self.rows]))

    def firth(self, var_idx, flip, mean, maxit=50):
        var_idx = np.asarray(var_idx, dtype=np.int64)
        RefDsScanner.calls.append((np.asarray(self.sc.sm.mu).copy(), var_idx.size))
        return firth_ds_ref(self.sc.sm, self.rows[var_idx], flip, mean)

    def close(self):
        self.rows = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RefDsScanner(R.RefScanner):
    """``RefScanner`` plus the dosage scans of the CPU oracle and ``dosage_block``."""

    calls = []           # (mu of the model, number of rows) of every DosageBlock.firth call, for the tests
    block_type = _RefDsBlock

    def scan_f64(self, dosage):
        return self._o.scan_f64(dosage)

    def scan_u8(self, dosage):
        return self._o.scan_u8(dosage)

    def dosage_block(self, dtype, max_variants):
        return self.block_type(self, dtype, max_variants)
