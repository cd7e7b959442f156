"""Reference of sgx_ds_block_cond_set / sgx_ds_block_cond -- TEST INFRASTRUCTURE ONLY.

The dosage twin of tests/cond_ref.py: G comes from ``skat_ds_ref.dosage_G`` (dosage rows, ``flip`` and ``mean`` exactly
as the entries are defined), then the algebra of ``cond_ref.cond_ref`` on the dense adjusted genotypes
adj = G - (G XV) XXVX_inv', in ``np.longdouble`` by default:
    S_j = sum_i (y - mu)_i adj_ji,   Phi_jl = r sum_i mu2_i adj_ji adj_li        (quantitative: mu2 = 1, S / tau[0])
and the conditional test formed directly from the residual row adj_j - b adj_C.

``NumpyCondDsScanner`` is ``skat_ds_ref.NumpySkatDsScanner`` whose dosage block gains ``cond_set`` / ``cond`` in double,
so that the dosage route of ``seqAssocGLMM_SPA_cond`` runs without a GPU.
"""
import dataclasses

import numpy as np

import cond_ref as CR
from skat_ds_ref import NumpySkatDsScanner, _NumpySkatDosageBlock, dosage_G


def cond_ds_ref(sm, rows, flip, mean, rows_c, flip_c, mean_c, dtype=np.longdouble):
    """rows [m, n] with flip / mean per row; rows_c [C, n] the conditioning rows with theirs.
    -> dict as ``cond_ref.cond_ref``: S, var, cov, S_C, Phi_CC, T, V in ``dtype``."""
    return cond_G_ref(sm, lambda a, b: dosage_G(rows[a:b], np.arange(b - a), flip[a:b], mean[a:b], dtype), len(rows),
                      dosage_G(rows_c, np.arange(len(rows_c)), flip_c, mean_c, dtype), dtype)


def cond_G_ref(sm, G_of, m, G_c, dtype=np.longdouble):
    """The algebra of ``cond_ref.cond_ref`` on dosage vectors: ``G_of(a, b)`` gives rows [a, b) of G, ``G_c`` the set's."""
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)
    mu2 = np.ones(sm.n, dtype=dtype) if sm.quant else np.asarray(sm.mu2, dtype=dtype)
    y_mu = np.asarray(sm.y_mu, dtype=dtype)
    if sm.quant:
        y_mu = y_mu / dtype(sm.tau[0])
    r = dtype(sm.var_ratio)
    c = G_c.shape[0]
    adj_of = lambda G: G - (G @ XV) @ XXVXi.T      # noqa: E731
    aC = adj_of(np.asarray(G_c, dtype=dtype))
    wC = aC * mu2
    gram = wC @ aC.T
    out = dict(S_C=aC @ y_mu, Phi_CC=r * gram)
    S, var, T, V = (np.zeros(m, dtype=dtype) for _ in range(4))
    cov = np.zeros((m, c), dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j0 in range(0, m, 64):                  # (in pieces: a long-double row of N = 70 001 is 1.1 MB)
            a = adj_of(np.asarray(G_of(j0, min(m, j0 + 64)), dtype=dtype))
            s = slice(j0, j0 + a.shape[0])
            S[s], var[s], cov[s] = a @ y_mu, r * np.sum(a * a * mu2, axis=1), r * (a @ wC.T)
            b = CR.solve(gram, wC @ a.T).T          # [rows, C]
            res = a - b @ aC
            T[s], V[s] = res @ y_mu, r * np.sum(res * res * mu2, axis=1)
    out.update(S=S, var=var, cov=cov, T=T, V=V)
    return out


class _NumpyCondDosageBlock(_NumpySkatDosageBlock):
    def cond_set(self, var_idx, flip, mean):
        var_idx = np.asarray(var_idx, dtype=np.int64)
        c = var_idx.size
        # the set belongs to the scanner: it outlives this block
        self.sc.cond_G = dosage_G(self.rows, var_idx, flip, mean, np.float64)
        S, cov = self.skat([0, c], var_idx, flip, mean)
        self.sc.cond_S, self.sc.cond_Phi = np.array(S), np.array(cov[0])
        return self.sc.cond_S, self.sc.cond_Phi

    def cond(self, flip, mean):
        m = len(self.rows)
        r = cond_G_ref(self.sc._sm, lambda a, b: dosage_G(self.rows[a:b], np.arange(b - a), flip[a:b], mean[a:b], np.float64),
                       m, self.sc.cond_G, np.float64)
        self.sc.cond_log.append((r["S"], r["var"], r["cov"]))
        return r["S"], r["var"], r["cov"]


class NumpyCondDsScanner(NumpySkatDsScanner):
    """``NumpySkatDsScanner`` whose dosage block has ``cond_set`` / ``cond`` (cond_ds_ref in double), with the
    ``set_thresholds`` of the device scanner.  ``cond_log`` keeps what every ``cond`` call returned."""

    def __init__(self, sm):
        super().__init__(sm)
        self.cond_G = self.cond_S = self.cond_Phi = None
        self.cond_log = []

    def set_thresholds(self, maf, mac, missing, spa_pval):
        from oracle.oracle import Oracle
        sm = dataclasses.replace(self._sm, maf=maf, mac=mac, missing=missing, spa_pval=spa_pval)
        Oracle.close(self)
        Oracle.__init__(self, sm)
        self._sm = sm

    def dosage_block(self, dtype, max_variants):
        return _NumpyCondDosageBlock(self, dtype, max_variants)
