"""Reference of sgx_skat_kmat_2bit -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of the definition in two forms:

    Sigma = tau[0] diag(1/w) + tau[1] K,    Y = Sigma^-1 A,  Z = Sigma^-1 X,
    C = A'Y,  D = A'Z,  E = X'Z,            Phi^K = 1/2 (C + C') - D E^-1 D'

with A the columns adj_e = G_e - XXVX_inv (XV G_e) of tests/skat_ref.py:

* ``phi_f64``: float64, the solves by a plain preconditioned CG with the stopping rule of the device loop
  (``PCG_diag_sigma``: Jacobi preconditioner with the 1e-4 floor, stop at r'r <= tol or after maxiter steps);
* ``phi_ld``: ``np.longdouble``, the solves by a direct Cholesky factorisation of Sigma (block by block where K is
  block diagonal).

It also holds the case table of tests/test_gpu_skat_kmat.py, the input makers and the recorded tolerances.

Recorded on the CPU (tests/test_skat_kmat_ref.py::test_f64_against_long_double prints them), tol = 1e-12, maxiter = 500,
|dPhi_ef| / sqrt(Phi_ee Phi_ff) over the whole case table:

    largest discrepancy of phi_f64 against phi_ld   5.54e-8 (n61_k3_dense; 6e-16 .. 5e-8 over the cases): what a solve
                                                    stopped at r'r <= 1e-12 leaves, REF_DISCREPANCY
    bound of the device against phi_ld              PHI_TOL = 10 x that = 5.55e-7 (the margin: another summation order,
                                                    which may move a column's last step)

The float64 CG converges in every case (largest step count below maxiter: the same test asserts it).
"""
import numpy as np

import skat_ref as R

TOL_SOLVE, MAXITER = 1e-12, 500
# The tie to the fit (tests/test_gpu_skat_kmat.py check 4): Phi^K_jj / AC_j against var1 of the golden models'
# variance-ratio tables at tol = 1e-5, relative to var1.  Measured on the CPU with phi_f64 on the dense K = G'G/M of
# tests/test_fit_grm_mat.py (tests/test_skat_kmat_ref.py::test_tie_to_the_fit_on_the_cpu prints them): 1.72e-8 for the
# binary model (3 steps a column), 1.7e-15 for the quantitative one (tau[1] = 0).  The device is held to 10 x the larger.
FIT_DISCREPANCY = 1.72e-8
FIT_TOL = 10 * FIT_DISCREPANCY
REF_DISCREPANCY = 5.55e-8    # measured (5.54e-8, case n61_k3_dense): see the module docstring
PHI_TOL = 10 * REF_DISCREPANCY

# (name, N, covariates, trait, storage of K, unit sizes (0: an empty unit), tau)
# N: below one slab or wave / no multiple of 4, 16, 64 / more than one slab of 2048 samples of the products
# (4099 = 2 * 2048 + 3) / more than one slab of 8192 samples of the column sums (8195 = 8192 + 3);
# m: one tile, a tile edge, the 64-column chunk edge, three chunks with a ragged last one
CASES = [
    ("n61_k1_csr", 61, 1, "binary", "csr", (1, 2, 0, 17), (1.0, 0.5)),
    ("n61_k3_dense", 61, 3, "quantitative", "dense", (16, 0, 2), (0.8, 0.4)),
    ("n1003_k3_csr", 1003, 3, "binary", "csr", (64, 0, 65), (1.0, 0.5)),
    ("n1003_k5_dense", 1003, 5, "binary", "dense", (17, 0, 130), (1.0, 0.3)),
    ("n1003_k1_dense_q", 1003, 1, "quantitative", "dense", (1, 16), (0.7, 0.6)),
    ("n4099_k5_csr", 4099, 5, "quantitative", "csr", (2, 0, 130), (0.9, 0.5)),
    ("n4099_k3_csr_b", 4099, 3, "binary", "csr", (65, 16), (1.0, 0.8)),
    ("n8195_k3_csr", 8195, 3, "binary", "csr", (3, 0, 18), (1.0, 0.5)),
]
FAMILY_SIZES = (1, 2, 3, 40, 0, 5)      # 40 >= SGX_KMAT_WAVE_ROW entries in a row; 0: a sample with an empty row


def flat_model(n, kcov, trait):
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    mod = synth.synth_null_model(n, trait, 0.2, n_cov=kcov, seed=777 + n + kcov)
    return mod, init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))


def hard_calls(n, m, seed):
    """m rows of hard calls: about 2 % missing, every 5th row alt-major (flipped), row 1 (if there is one) all
    reference or missing: monomorphic after imputation."""
    rng = np.random.default_rng(seed)
    af = 10 ** rng.uniform(-1.5, -0.4, m)
    af[::5] = 1 - af[::5]
    codes = (rng.random((m, n)) < af[:, None]).astype(np.uint8) + (rng.random((m, n)) < af[:, None]).astype(np.uint8)
    if m > 1:
        codes[1] = 0
    codes[rng.random((m, n)) < 0.02] = 3
    return codes


def family_blocks(n):
    """Contiguous families of FAMILY_SIZES, cycled -> [(start, size)]; a size of 0 stands for one sample with no
    entry at all (not even a diagonal)."""
    out, i, k = [], 0, 0
    while i < n:
        s = FAMILY_SIZES[k % len(FAMILY_SIZES)]
        k += 1
        sz = min(max(s, 1), n - i)
        out.append((i, sz, s == 0))
        i += sz
    return out


def family_K(n):
    """Block-diagonal kinship: 1 on the diagonal, 0.5 within a family (positive definite per block) -> dense [n, n]
    float64, (row_ptr, col, val) of its full pattern, the blocks as index ranges."""
    K = np.zeros((n, n))
    blocks = []
    for i, sz, empty in family_blocks(n):
        if not empty:
            K[i:i + sz, i:i + sz] = 0.5 + 0.5 * np.eye(sz)
        blocks.append((i, i + sz))
    nz = K != 0
    row_ptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    col = np.nonzero(nz)[1].astype(np.int32)
    return K, (row_ptr, col, K[nz]), blocks


def dense_K(n, seed, n_marker=300):
    """G'G / M of standardised random markers: dense, positive semi-definite of rank <= M."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, n_marker)
    g = (rng.random((n_marker, n)) < af[:, None]).astype(np.float64) + (rng.random((n_marker, n)) < af[:, None])
    g = (g - 2 * af[:, None]) / np.sqrt(2 * af * (1 - af))[:, None]
    return np.ascontiguousarray(g.T @ g / n_marker)


_cases = {}


def fit_case(trait, K):
    """The tie to the fit: the golden model of ``trait``, the markers of its variance-ratio table as one unit of the
    golden file's rows, w = the model's V, tau the model's, K the dense G'G/M of the markers the fit picks ->
    (case as make_case's, AC [markers], var1 [markers] of the table)."""
    import os
    from conftest import GOLDEN, load_null_model, scan_model
    from saigegds_amd.gds import unpack_dosage_2bit
    name = "saige_model.npz" if trait == "binary" else "saige_model_quant.npz"
    z, g = np.load(os.path.join(GOLDEN, name)), np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    mod, sm = load_null_model(name), scan_model(name)
    assert list(mod.sample_id) == [str(v) for v in g["sample_id"]]
    pos = {int(v): k for k, v in enumerate(g["variant_id"])}
    packed = np.ascontiguousarray(g["packed"][[pos[int(v)] for v in z["vr_id"]]])
    m = packed.shape[0]
    c = dict(name="fit_" + trait, n=sm.n, kcov=sm.k, trait=trait, storage="dense", sm=sm, mod=mod, packed=packed,
             lut=R.tables(unpack_dosage_2bit(packed, sm.n)), var_idx=np.arange(m, dtype=np.int32),
             unit_ptr=np.array([0, m], dtype=np.int64), K=np.ascontiguousarray(K, dtype=np.float64), csr=None, blocks=None,
             w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.asarray(mod.tau, dtype=np.float64))
    return c, np.asarray(z["vr_mac"], dtype=np.float64), np.asarray(z["vr_var1"], dtype=np.float64)


def make_case(name):
    """The inputs of a case, made once: model, rows, tables, units, K (dense array, CSR or None, blocks or None), w, tau."""
    if name in _cases:
        return _cases[name]
    from saigegds_amd.gds import pack_dosage_2bit
    _, n, kcov, trait, storage, units, tau = next(c for c in CASES if c[0] == name)
    mod, sm = flat_model(n, kcov, trait)
    m_tot = int(sum(units))
    codes = hard_calls(n, m_tot, 31 + n + kcov)
    if storage == "csr":
        K, csr, blocks = family_K(n)
    else:
        K, csr, blocks = dense_K(n, 5 + n), None, None
    c = dict(name=name, n=n, kcov=kcov, trait=trait, storage=storage, sm=sm, mod=mod, codes=codes,
             packed=pack_dosage_2bit(codes), lut=R.tables(codes), var_idx=np.arange(m_tot, dtype=np.int32),
             unit_ptr=np.concatenate([[0], np.cumsum(units)]).astype(np.int64), K=K, csr=csr, blocks=blocks,
             w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.array(tau, dtype=np.float64))
    _cases[name] = c
    return c


def adj_columns(sm, packed, var_idx, lut, dtype):
    """A [entries, N]: adj_e = G_e - XXVX_inv (XV G_e), and the score statistics S_e (quantitative: / tau[0])."""
    G = R.dosage_rows(packed, sm.n, var_idx, lut, dtype)
    XV, XXVXi = np.asarray(sm.XV, dtype=dtype), np.asarray(sm.t_XXVX_inv, dtype=dtype)
    A = G - (G @ XV) @ XXVXi.T
    S = A @ np.asarray(sm.y_mu, dtype=dtype)
    return A, (S / dtype(sm.tau[0]) if sm.quant else S)


def pcg_f64(K, w, tau, B, maxiter, tol):
    """PCG_diag_sigma on the rows of B in float64 -> (X, iters): every column on its own scalars."""
    w, B = np.asarray(w, dtype=np.float64), np.asarray(B, dtype=np.float64)
    minv = 1.0 / np.maximum(tau[0] / w + tau[1] * np.diag(K), 1e-4)
    X, Rr = np.zeros_like(B), B.copy()
    Zz = Rr * minv
    P = Zz.copy()
    rr, rz = (Rr * Rr).sum(axis=1), (Rr * Zz).sum(axis=1)
    iters = np.zeros(B.shape[0], dtype=np.int32)
    while True:
        act = np.nonzero((iters < maxiter) & (rr > tol))[0]
        if act.size == 0:
            return X, iters
        iters[act] += 1
        Pa = P[act]
        AP = tau[0] * (Pa / w) + (tau[1] * (Pa @ K) if tau[1] != 0 else 0.0)
        a = rz[act] / (Pa * AP).sum(axis=1)
        X[act] += a[:, None] * Pa
        Rr[act] -= a[:, None] * AP
        Zz[act] = Rr[act] * minv
        rz1 = (Zz[act] * Rr[act]).sum(axis=1)
        rr[act] = (Rr[act] * Rr[act]).sum(axis=1)
        P[act] = Zz[act] + (rz1 / rz[act])[:, None] * Pa
        rz[act] = rz1


def _chol_solve_ld(S, B):
    """S x = b for the columns of B [n, k] by Cholesky in long double."""
    n = S.shape[0]
    L = np.array(S, dtype=np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.array(B, dtype=np.longdouble)
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


def solve_ld(K, w, tau, B, blocks=None):
    """Sigma^-1 applied to the rows of B in long double; ``blocks``: index ranges K is block diagonal over."""
    ld = np.longdouble
    n = K.shape[0]
    out = np.zeros(np.shape(B), dtype=ld)
    Bt = np.asarray(B, dtype=ld).T
    for i0, i1 in (blocks or [(0, n)]):
        S = ld(tau[1]) * np.asarray(K[i0:i1, i0:i1], dtype=ld)
        S[np.diag_indices(i1 - i0)] += ld(tau[0]) / np.asarray(w[i0:i1], dtype=ld)
        out[:, i0:i1] = _chol_solve_ld(S, Bt[i0:i1]).T
    return out


def _phi(A, X, Y, Z, dtype):
    C, D, E = A @ Y.T, A @ Z.T, X @ Z.T
    Ei = np.linalg.inv(np.asarray(0.5 * (E + E.T), dtype=np.float64)).astype(dtype) if dtype is np.float64 \
        else _chol_solve_ld(0.5 * (E + E.T), np.eye(E.shape[0], dtype=dtype))
    phi = 0.5 * (C + C.T) - D @ (0.5 * (Ei + Ei.T)) @ D.T
    return 0.5 * (phi + phi.T)


def phi_units(c, form, tol=TOL_SOLVE, maxiter=MAXITER, tau=None):
    """The reference of a case in one of its two forms ("f64" / "ld") -> (score [entries], [Phi^K of unit u], iters)."""
    dtype = np.float64 if form == "f64" else np.longdouble
    tau = c["tau"] if tau is None else np.asarray(tau, dtype=np.float64)
    sm = c["sm"]
    A, S = adj_columns(sm, c["packed"], c["var_idx"], c["lut"], dtype)
    X = np.asarray(sm.t_X, dtype=dtype).T
    if form == "f64":
        Z, _ = pcg_f64(c["K"], c["w"], tau, X, maxiter, tol)
        Y, iters = pcg_f64(c["K"], c["w"], tau, A, maxiter, tol)
    else:
        Z = solve_ld(c["K"], c["w"], tau, X, c["blocks"])
        Y, iters = solve_ld(c["K"], c["w"], tau, A, c["blocks"]), None
    up = c["unit_ptr"]
    return S, [_phi(A[up[u]:up[u + 1]], X, Y[up[u]:up[u + 1]], Z, dtype) for u in range(len(up) - 1)], iters


def scaled_error(cov, ref):
    """max |cov_ef - ref_ef| / sqrt(ref_ee ref_ff); an entry of variance 0 (a monomorphic row: adj = 0 exactly) must
    be matched exactly and counts as 0 / inf."""
    ref = np.asarray(ref, dtype=np.longdouble)
    if ref.size == 0:
        return 0.0
    sd = np.sqrt(np.maximum(np.diag(ref), 0))
    d = np.abs(np.asarray(cov, dtype=np.longdouble) - ref)
    sc = sd[:, None] * sd[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(sc > 0, d / sc, np.where(d == 0, 0.0, np.inf))
    return float(e.max())


def chunk_case(m, seed):
    """The inputs of the tests that cut the host rows into chunks: N = 70 001, K = 2 covariates, m rows of hard calls,
    and a GRM of pairs (1 on the diagonal, 0.5 between samples 2i and 2i + 1; the last sample alone) as CSR, so that
    the solves are trivial.  Made once per (m, seed)."""
    key = ("chunk", m, seed)
    if key not in _cases:
        from saigegds_amd.gds import pack_dosage_2bit
        n = 70001
        mod, sm = flat_model(n, 2, "binary")
        assert sm.k == 2
        codes = hard_calls(n, m, seed)
        from skat_ref import tables
        i = np.arange(n)
        mate = i ^ 1
        cols = np.stack([np.minimum(i, mate), np.maximum(i, mate)], axis=1)
        keep = cols < n
        row_ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
        val = np.where(cols == i[:, None], 1.0, 0.5)
        _cases[key] = dict(sm=sm, packed=pack_dosage_2bit(codes), lut=tables(codes), storage="csr", K=None,
                           csr=(row_ptr, cols[keep].astype(np.int32), val[keep]),
                           w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.array([1.0, 0.5]))
    return _cases[key]
