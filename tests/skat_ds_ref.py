"""Reference of sgx_ds_block_skat -- TEST INFRASTRUCTURE ONLY.

The dosage twin of tests/skat_ref.py: G is built from dosage rows, ``flip`` and ``mean`` exactly as the entry is defined,
    g_e(i) = present(x) ? (flip[e] ? 2 - x : x) : mean[e],      x = rows[var_idx[e]][i]
(uint8: 0xFF missing; int32: NA_INTEGER missing; float64: non-finite missing), then the dense-branch algebra of
``skat_ref.skat_ref`` -- independent of the kernel's carrier-sum algebra -- in ``np.longdouble`` by default:
    adj = G - (G XV) XXVX_inv',    Phi = r (adj mu2) adj',    S = adj (y - mu)    (quantitative: mu2 = 1, S / tau[0]).
Every unit is computed from its own entries alone.

``NumpySkatDsScanner`` gives the SKAT driver a dosage block with a ``skat`` method in numpy (float64), so that its host
logic runs without a GPU.
"""
import numpy as np

from aggregate_ds_ref import NumpyDsScanner, _NumpyDosageBlock, ok_mask


def dosage_G(rows, var_idx, flip, mean, dtype=np.longdouble):
    """G [entries, n] in ``dtype``."""
    rows = np.asarray(rows)
    G = np.zeros((len(var_idx), rows.shape[1]), dtype=dtype)
    for e, v in enumerate(np.asarray(var_idx, dtype=np.int64)):
        row = rows[v]
        ok = ok_mask(row)
        x = np.where(ok, row, 0).astype(dtype)
        G[e] = np.where(ok, 2 - x if flip[e] else x, dtype(mean[e]))
    return G


def skat_ds_ref(sm, rows, unit_ptr, var_idx, flip, mean, dtype=np.longdouble):
    """-> (score [entries], [cov of unit u: (m_u, m_u)]) in ``dtype``."""
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)      # [N, K] both
    mu2 = np.ones(sm.n, dtype=dtype) if sm.quant else np.asarray(sm.mu2, dtype=dtype)
    y_mu = np.asarray(sm.y_mu, dtype=dtype)
    var_idx, flip, mean = np.asarray(var_idx), np.asarray(flip), np.asarray(mean, dtype=np.float64)
    score, cov = np.zeros(var_idx.size, dtype=dtype), []
    with np.errstate(invalid="ignore"):
        for u in range(len(unit_ptr) - 1):
            a, b = int(unit_ptr[u]), int(unit_ptr[u + 1])
            G = dosage_G(rows, var_idx[a:b], flip[a:b], mean[a:b], dtype)
            adj = G - (G @ XV) @ XXVXi.T
            s = adj @ y_mu
            score[a:b] = s / dtype(sm.tau[0]) if sm.quant else s
            cov.append(dtype(sm.var_ratio) * ((adj * mu2) @ adj.T))
    return score, cov


def flip_mean(rows):
    """(flip, mean) per row as the SKAT driver forms them: from n non-missing and their double sum s, flip = s > n,
    mean = s / n or 2 - s / n."""
    rows = np.asarray(rows)
    ok = np.stack([ok_mask(r) for r in rows])
    n = ok.sum(axis=1).astype(np.float64)
    s = np.where(ok, rows, 0).astype(np.float64).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s / n
    fl = s > n
    return fl.astype(np.uint8), np.where(fl, 2 - m, m)


class _NumpySkatDosageBlock(_NumpyDosageBlock):
    def skat(self, unit_ptr, var_idx, flip, mean):
        self.sc.skat_calls += 1
        return skat_ds_ref(self.sc._sm, self.rows, unit_ptr, var_idx, flip, mean, dtype=np.float64)


class NumpySkatDsScanner(NumpyDsScanner):
    """``NumpyDsScanner`` whose dosage block has ``skat`` (skat_ds_ref in double); counts the skat calls."""

    def __init__(self, sm):
        super().__init__(sm)
        self._sm, self.skat_calls = sm, 0

    def dosage_block(self, dtype, max_variants):
        return _NumpySkatDosageBlock(self, dtype, max_variants)
