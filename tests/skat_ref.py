"""Reference of sgx_skat_2bit -- TEST INFRASTRUCTURE ONLY.

Independent of the kernel's algebra (carrier sums against the flattened score columns): the dense
adjusted genotype of the single-variant test's dense branch, from the model's own XV and XXVX_inv,
    adj_j = G_j - XXVX_inv (XV G_j),    Phi_jl = r sum_i mu2_i adj_ji adj_li,    S_j = sum_i (y - mu)_i adj_ji
(quantitative traits: mu2 = 1 and S / tau[0]), in ``np.longdouble`` by default.
"""
import numpy as np


def dosage_rows(packed, n, var_idx, lut, dtype=np.longdouble):
    """G [entries, n]: the table of every entry looked up at the 2-bit codes of its variant."""
    from saigegds_amd.gds import unpack_dosage_2bit
    var_idx = np.asarray(var_idx, dtype=np.int64)
    rows = np.unique(var_idx)
    codes = dict(zip(rows.tolist(), unpack_dosage_2bit(np.ascontiguousarray(np.asarray(packed)[rows], dtype=np.uint8), n)))
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 4)
    return np.stack([lut[e].astype(dtype)[codes[int(v)]] for e, v in enumerate(var_idx)]) if var_idx.size \
        else np.zeros((0, n), dtype=dtype)


def skat_ref(sm, packed, unit_ptr, var_idx, lut, dtype=np.longdouble):
    """-> (score [entries], [cov of unit u: (m_u, m_u)]) in ``dtype``."""
    G = dosage_rows(packed, sm.n, var_idx, lut, dtype)
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)      # [N, K] both
    adj = G - (G @ XV) @ XXVXi.T
    mu2 = np.ones(sm.n, dtype=dtype) if sm.quant else np.asarray(sm.mu2, dtype=dtype)
    score = adj @ np.asarray(sm.y_mu, dtype=dtype)
    if sm.quant:
        score = score / dtype(sm.tau[0])
    cov = []
    for u in range(len(unit_ptr) - 1):
        a = adj[int(unit_ptr[u]):int(unit_ptr[u + 1])]
        cov.append(dtype(sm.var_ratio) * ((a * mu2) @ a.T))
    return score, cov


def hard_calls(n, m, seed):
    """Hard calls as tests/test_gpu_aggregate_dosage.py makes them: 1 % missing, every 7th row alt-major."""
    rng = np.random.default_rng(seed)
    af = 10 ** rng.uniform(-2.3, -0.4, m)
    af[::7] = 1 - af[::7]
    codes = (rng.random((m, n)) < af[:, None]).astype(np.uint8) + (rng.random((m, n)) < af[:, None]).astype(np.uint8)
    codes[rng.random((m, n)) < 0.01] = 3
    return codes


def tables(codes):
    """Unweighted dosage tables {0, 1, 2, m} / {2, 1, 0, 2 - m} of the rows, as the drivers build them."""
    ok = codes != 3
    n = ok.sum(axis=1).astype(np.float64)
    s = np.where(ok, codes, 0).sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s / n
    z = 0 * m
    return np.where((s > n)[:, None], np.stack([2 + z, 1 + z, z, 2 - m], axis=1), np.stack([z, 1 + z, 2 + z, m], axis=1))
