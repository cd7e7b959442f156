"""Long-double reference of the leave-one-group-out GRM operator, on top of grm_ref.py, with the group
layouts and inputs that test_gpu_grm_loco.py uses.  No test functions here.

Leaving group c out of the GRM is the operator of the markers outside c: af_v and inv_v are per marker, so
    out = G_c'(G_c b) / (M - M_c),    diag_excl[c] = diag of that operator,
G_c being the rows of G whose group is not c.  reference_loco() states it that way, through
grm_ref.reference() on the remaining rows; excl = -1 keeps every row.

pcg_reference() is PCG_diag_sigma (reference src/saige_fitnull.cpp:581-614) in plain numpy, every column with
its own w and its own operator, the operator applied in long double and rounded to double.
"""
import numpy as np

import grm_ref as R

LD = R.LD


def keep_rows(group, excl):
    group = np.asarray(group)
    return np.ones(group.size, dtype=bool) if excl < 0 else group != excl


def reference_loco(codes, group, B, excl):
    """B: [k, n], excl: [k] -> Ref(out [k, n], diag [k, n], scale [k, n]) in np.longdouble; row j on the markers
    outside group excl[j]."""
    B = np.asarray(B, dtype=np.float64)
    excl = np.asarray(excl)
    out = np.zeros(B.shape, dtype=LD)
    diag = np.zeros(B.shape, dtype=LD)
    scale = np.zeros(B.shape, dtype=LD)
    for c in np.unique(excl):
        rows = np.flatnonzero(excl == c)
        ref = R.reference(np.asarray(codes)[keep_rows(group, c)], B[rows])
        out[rows], diag[rows], scale[rows] = ref.out, ref.diag[None, :], ref.scale
    return R.Ref(out, diag, scale)


def diag_excl(codes, group, c):
    """[n] np.longdouble: the diagonal of the GRM of the markers outside group c."""
    codes = np.asarray(codes)
    return R.reference(codes[keep_rows(group, c)], np.zeros(codes.shape[1])).diag


def _std_geno(codes):
    af, inv = R.marker_stats(codes)
    return np.where(codes != 3, (codes.astype(LD) - 2 * af.astype(LD)[:, None]) * inv.astype(LD)[:, None], LD(0))


def pcg_reference(codes, group, W, w_idx, tau, B, excl, maxiter, tol):
    """-> X [k, n] float64, iters [k].  Column j: (tau0 diag(1 / W[w_idx[j]]) + tau1 GRM without excl[j]) x = B[j]."""
    codes = np.asarray(codes)
    B = np.asarray(B, dtype=np.float64)
    g_all = _std_geno(codes)
    tau0, tau1 = float(tau[0]), float(tau[1])
    X = np.zeros_like(B)
    iters = np.zeros(B.shape[0], dtype=np.int64)
    for j in range(B.shape[0]):
        g = g_all[keep_rows(group, excl[j])]
        m = LD(g.shape[0])
        w = np.asarray(W[w_idx[j]], dtype=np.float64)
        diag = ((g * g).sum(axis=0) / m).astype(np.float64)

        def grm(p):
            return ((g.T @ (g @ p.astype(LD))) / m).astype(np.float64)

        minv = 1 / np.maximum(tau0 / w + tau1 * diag, 1e-4)
        r = B[j].copy()
        z = minv * r
        p = z.copy()
        x = np.zeros_like(r)
        rz, rr, it = float(r @ z), float(r @ r), 0
        while it < maxiter and rr > tol:
            it += 1
            Ap = tau0 * (p / w)
            if tau1 != 0:
                Ap = Ap + tau1 * grm(p)
            a = rz / float(p @ Ap)
            x += a * p
            r -= a * Ap
            z = minv * r
            rz1 = float(z @ r)
            p = z + (rz1 / rz) * p
            rz, rr = rz1, float(r @ r)
        X[j], iters[j] = x, it
    return X, iters


# ---- group layouts: name -> (group [m] int32, n_groups)
LAYOUTS = ("contig", "interleaved", "empty", "big")


def layout(name, m):
    v = np.arange(m)
    if name == "contig":          # boundaries inside a 16-marker dword and inside a 256-row tile
        edges = [7, min(100, m // 2), (3 * m) // 5 | 1]
        assert all(e % 16 for e in edges) and all(0 < e < m for e in edges) and edges == sorted(set(edges))
        return np.searchsorted(edges, v, side="right").astype(np.int32), 4
    if name == "interleaved":
        return (v % 3).astype(np.int32), 3
    if name == "empty":           # group 1 holds no marker
        return np.array([0, 2, 3], dtype=np.int32)[v % 3], 4
    if name == "big":             # group 0 holds all but a handful
        g = np.zeros(m, dtype=np.int32)
        g[[1, m // 3, m // 3 + 1, m // 2, m - 2]] = 1
        return g, 2
    raise KeyError(name)


LOCO_SHAPES = [(257, 255), (513, 511), (255, 257)]


def zero_diag_case(n, m):
    """Codes and groups where leaving group 1 out leaves sample 0 with every remaining code missing, while the
    whole GRM has diag_0 > 0."""
    codes = np.array(R.case(n, m, 5e-3).codes)
    group = (np.arange(m) % 3).astype(np.int32)
    codes[group != 1, 0] = 3
    assert np.any((codes[group == 1, 0] != 3) & (R.marker_stats(codes)[1][group == 1] > 0))
    return codes, group, 3
