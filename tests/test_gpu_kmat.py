"""The explicit-matrix operator on the device (sgx_kmat, ``ExplicitGrmOperator``): CSR and dense products against
the long-double reference at the bound of kmat_ref.py, the bit identities of a column, and the solve."""
import functools
import os

import numpy as np
import pytest

import kmat_ref as KR
from saigegds_amd._lib import GRM_MAX_RHS, KMAT_WAVE_ROW, ExplicitGrmOperator, GrmOperator, SgxError

pytestmark = pytest.mark.gpu

T = KMAT_WAVE_ROW - 1          # the longest row of the thread form
CSR_N = (1, 63, 64, 65, 257, 1000)
DENSE_N = (1, 15, 16, 17, 63, 65, 130, 1000, 1030, 2049)    # 1030, 2049: two and three column slabs of the kernel
KS = (1, 2, 16, 17, 64)


SPECIAL = {100: T - 1, 140: T, 180: T + 1}      # row -> stored entries, around the thread / wave switch
FULL, EMPTY, NO_DIAG = 220, 7, 30


@functools.lru_cache(maxsize=None)
def csr_case(n):
    """Upper triangle of a symmetric matrix of families of 1..5 (diagonal-only rows among them), and, where n
    allows: row NO_DIAG without its diagonal entry (n >= 63), rows of T - 1, T, T + 1 entries (n >= 257), one full
    row (n = 257) or one empty row (the other n >= 63: a full row leaves none empty)."""
    rng = np.random.default_rng([n, 17])
    i, j, x = KR.family_matrix(n, 21)
    ent = {(int(a), int(b)): float(v) for a, b, v in zip(i, j, x)}

    def clear(r):
        for e in [k for k in ent if r in k]:
            del ent[e]

    full = n == 257
    if n >= 257:
        keep_out = set(SPECIAL) | {FULL, EMPTY}
        others = [c for c in range(n) if c not in keep_out]
        for r in SPECIAL:
            clear(r)
        for r, length in SPECIAL.items():
            ent[(r, r)] = 1.05
            for c in rng.choice(others, length - 1 - int(full), replace=False):
                ent[(min(r, int(c)), max(r, int(c)))] = float(rng.uniform(-0.5, 0.5))
    if full:
        clear(FULL)
        for c in range(n):
            ent[(min(FULL, c), max(FULL, c))] = 1.05 if c == FULL else float(rng.uniform(-0.5, 0.5))
    elif n >= 63:
        clear(EMPTY)
    if n >= 63:
        ent.pop((NO_DIAG, NO_DIAG), None)
        ent[(NO_DIAG, NO_DIAG + 1)] = 0.25
    keys = sorted(ent)
    up = KR.Upper(n, [k[0] for k in keys], [k[1] for k in keys], [ent[k] for k in keys])
    r, c, v = KR.full_pattern(n, up.i, up.j, up.x)
    return up, KR.csr_of(n, r, c, v)


def test_csr_case_has_the_rows_it_names():
    for n in (257, 1000):
        up, (rp, col, val) = csr_case(n)
        nnz = np.diff(rp)
        assert [int(nnz[r]) for r in SPECIAL] == list(SPECIAL.values())
        assert NO_DIAG not in col[rp[NO_DIAG]:rp[NO_DIAG + 1]] and nnz[NO_DIAG] > 0
        assert nnz[FULL] == n if n == 257 else nnz[EMPTY] == 0
    assert (nnz == 1).any() and {2, 3, 4, 5} <= set(int(v) for v in nnz)         # (n = 1000: diagonal-only rows, families)
    assert np.diff(csr_case(64)[1][0])[EMPTY] == 0


@functools.lru_cache(maxsize=None)
def rhs(n, k=64):
    B = np.random.default_rng([n, 5]).standard_normal((k, n))
    B[1] = 1.0
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def dense_case(n):
    rng = np.random.default_rng([n, 31])
    A = rng.standard_normal((n, n))
    K = (A + A.T) / 2 + np.diag(rng.uniform(1, 2, n))
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def dense_ref(n):
    return KR.dense_product_ld(dense_case(n), rhs(n))


def check_columns(op, B, ref, amp, nterms):
    """The products of B's rows: the bound, and the bit identities of a column."""
    n = B.shape[1]
    one = np.stack([op.crossprod(b) for b in B[:3]])
    KR.assert_within_bound(one, ref[:3], amp[:3], nterms, "single")
    for k in KS:
        out = op.crossprod_many(B[:k])
        KR.assert_within_bound(out, ref[:k], amp[:k], nterms, f"k={k}")
        assert np.array_equal(out[:min(k, 3)], one[:min(k, 3)]), k          # column j of a multi call = the single call
    again = op.crossprod_many(B[:17])
    assert np.array_equal(again, op.crossprod_many(B[:17]))                # two calls
    mixed = np.stack([B[40], B[2], B[41], B[0]] + [B[50 + q] for q in range(14)] + [B[1]])   # other companions, places
    got = op.crossprod_many(mixed)
    assert np.array_equal(got[1], one[2]) and np.array_equal(got[3], one[0]) and np.array_equal(got[18], one[1])
    # ldb = n + 5 through the device form of the C entry: columns at a stride the host form packs away
    import torch
    Bd = torch.zeros((17, n + 5), dtype=torch.float64, device="cuda")
    Bd[:, :n] = torch.from_numpy(B[:17].copy()).cuda()
    Od = torch.full((17, n + 5), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    op.crossprod_many_dev(Bd.data_ptr(), n + 5, 17, Od.data_ptr())
    op.sync()
    O = Od.cpu().numpy()
    assert np.array_equal(O[:, :n], again) and (O[:, n:] == 7.0).all()
    assert op.matvec_ms() >= 0


@pytest.mark.parametrize("n", CSR_N)
def test_csr_products(n):
    up, (rp, col, val) = csr_case(n)
    B = rhs(n)
    ref, amp, nnz = KR.csr_product_ld(n, rp, col, val, B)
    dg = np.zeros(n)
    dg[up.i[up.i == up.j]] = up.x[up.i == up.j]
    with ExplicitGrmOperator(up) as op:
        assert op.storage == "csr" and np.array_equal(op.diag(), dg)
        check_columns(op, B, ref, amp, nnz)
    from saigegds_amd import SparseGRM
    sp = SparseGRM(sample_id=[str(k) for k in range(n)], n=n, n_markers=0, rel_cutoff=0.0, i=up.i, j=up.j, x=up.x)
    KR.assert_within_bound(np.stack([sp.matvec(b) for b in B[:3]]), ref[:3], amp[:3], nnz, "SparseGRM.matvec")


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_products(n, pad):
    K = dense_case(n)
    B = rhs(n)
    ref, amp = dense_ref(n)
    Kw = np.full((n, n + pad), np.nan)                  # (what lies beyond a row's n entries must not be read)
    Kw[:, :n] = K
    with ExplicitGrmOperator(Kw, ld=n + pad) as op:
        assert op.storage == "dense" and op.n == n and np.array_equal(op.diag(), np.diag(K))
        check_columns(op, B, ref, amp, n)


@pytest.mark.parametrize("n", [65, 257])
def test_csr_of_a_dense_matrix_agrees_with_dense_storage(n):
    K = dense_case(n)
    i, j = np.triu_indices(n)
    B = rhs(n)[:5]
    ref, amp = KR.dense_product_ld(K, B)
    with ExplicitGrmOperator(KR.Upper(n, i, j, K[i, j])) as a, ExplicitGrmOperator(K) as b:
        ya, yb = a.crossprod_many(B), b.crossprod_many(B)
    assert np.all(np.abs(ya - yb) <= 2 * (n + 2) * KR.U * amp.astype(np.float64))
    KR.assert_within_bound(ya, ref, amp, n)


@functools.lru_cache(maxsize=None)
def psd_case(n, big):
    up = KR.Upper(n, *KR.family_matrix(n, 9, big))
    rng = np.random.default_rng([n, 41])
    w = rng.uniform(0.05, 0.25, n)
    B = rng.standard_normal((5, n))
    B[1] = 1.0
    return up, w, B


@pytest.mark.parametrize("storage", ["csr", "dense"])
@pytest.mark.parametrize("n,big", [(65, 0), (1000, 80)])
def test_pcg(n, big, storage):
    up, w, B = psd_case(n, big)
    ref = KR.KmatRef(up)
    with ExplicitGrmOperator(up if storage == "csr" else up.to_dense()) as op:
        for tau in ([1.0, 0.5], [0.3, 0.7]):
            X, its = op.pcg_many(w, tau, B, 500, 1e-5)
            for c in range(B.shape[0]):
                xr, _ = ref.pcg(w, tau, B[c], 500, 1e-5)
                np.testing.assert_allclose(X[c], xr, rtol=1e-8, atol=1e-10 * np.max(np.abs(xr)))
                x1, it1 = op.pcg(w, tau, B[c], 500, 1e-5)
                assert np.array_equal(x1, X[c]) and it1 == its[c]
        # a column that starts converged leaves at once; the others are not disturbed
        B2 = B.copy()
        B2[2] = 1e-9
        X2, it2 = op.pcg_many(w, [1.0, 0.5], B2, 500, 1e-5)
        X1, it1 = op.pcg_many(w, [1.0, 0.5], B, 500, 1e-5)
        assert it2[2] == 0 and np.array_equal(X2[2], np.zeros(n))
        assert np.array_equal(np.delete(X2, 2, 0), np.delete(X1, 2, 0)) and np.array_equal(np.delete(it2, 2), np.delete(it1, 2))
        _, it3 = op.pcg_many(w, [1.0, 5.0], B, 3, 1e-30)
        assert (it3 == 3).all()
        # tau1 = 0, any w: one step x = a p with p = (1 / (tau0 / w)) b (three roundings against the two of
        # b w / tau0) and a = rz / pAp = 1 up to the roundings of two sums of n nearly equal terms: a tree of at
        # most 12 levels and a few host additions each.  64 units of 2^-53 cover both.
        X0, it0 = op.pcg_many(w, [0.8, 0.0], B, 500, 1e-5)
        assert (it0 == 1).all() and np.all(np.abs(X0 - B * w / 0.8) <= 64 * KR.U * np.abs(B * w / 0.8))


def test_tau1_zero_is_the_scaled_right_hand_side():
    """tau1 = 0 returns b w / tau0 to the last bit of that expression's double evaluation.  The loop is the implicit
    operator's (1 / (tau0 / w), then a = rz / pAp), so the bits are those of b w / tau0 where its own operations
    are exact, as with w = 1/4 and tau0 = 1/2; for any other w the rounding differs (test_pcg bounds it)."""
    up, w, B = psd_case(65, 0)
    w2 = np.full(65, 0.25)
    with ExplicitGrmOperator(up) as op:
        X, it = op.pcg_many(w2, [0.5, 0.0], B, 500, 1e-5)
    assert np.array_equal(X, B * w2 / 0.5)


def test_argument_errors():
    up, (rp, col, val) = csr_case(65)
    n = 65

    def bad(**kw):
        with pytest.raises(SgxError) as e:
            ExplicitGrmOperator(**kw)
        assert e.value.code == -1, kw                 # SGX_EINVAL

    c2 = col.copy(); c2[rp[3]], c2[rp[3] + 1] = c2[rp[3] + 1], c2[rp[3]]
    bad(csr=(rp, c2, val))                             # unsorted
    c3 = col.copy(); c3[rp[3] + 1] = c3[rp[3]]
    bad(csr=(rp, c3, val))                             # duplicate
    c4 = col.copy(); c4[-1] = n
    bad(csr=(rp, c4, val))
    c5 = col.copy(); c5[0] = -1
    bad(csr=(rp, c5, val))
    r2 = rp.copy(); r2[4] = r2[3] - 1
    bad(csr=(r2, col, val))
    v2 = val.copy(); v2[5] = np.inf
    bad(csr=(rp, col, v2))
    v2[5] = np.nan
    bad(csr=(rp, col, v2))
    bad(csr=(np.zeros(1, dtype=np.int64), col[:0], val[:0]), n=0)
    bad(grm=np.eye(4), n=0)
    bad(grm=np.eye(4), ld=3)
    import ctypes as C
    from saigegds_amd._lib import load
    L = load()
    with ExplicitGrmOperator(up) as op:
        B = np.zeros((GRM_MAX_RHS + 1, n + 2))
        O = np.zeros_like(B)
        w = np.ones(n)
        tau = np.array([1.0, 0.5])
        it = np.zeros(GRM_MAX_RHS + 1, dtype=np.int32)
        for k, ldb in ((0, n), (GRM_MAX_RHS + 1, n), (1, n - 1)):
            assert L.sgx_kmat_crossprod_multi(op._h, B.ctypes.data, ldb, k, O.ctypes.data) == -1
            assert L.sgx_kmat_crossprod_multi_dev(op._h, B.ctypes.data, ldb, k, O.ctypes.data) == -1
            assert L.sgx_kmat_pcg_multi(op._h, w.ctypes.data, tau.ctypes.data, B.ctypes.data, ldb, k, 5, 1e-5,
                                        O.ctypes.data, it.ctypes.data) == -1
        assert L.sgx_kmat_crossprod_multi(op._h, None, n, 1, O.ctypes.data) == -1
        assert L.sgx_kmat_pcg_multi(op._h, None, tau.ctypes.data, B.ctypes.data, n, 1, 5, 1e-5, O.ctypes.data,
                                    it.ctypes.data) == -1
        assert L.sgx_kmat_diag(op._h, None) == -1
        with pytest.raises(ValueError):
            op.crossprod(np.zeros(n + 1))
    # the dense budget: 8 n^2 bytes above 8 GiB is refused before anything is read
    assert L.sgx_kmat_init_dense(np.zeros(1).ctypes.data, 32769, 32769, 0, C.byref(C.c_void_p())) == -1


def test_implicit_operator_multi_solve_still_equals_single_solves():
    """The loop moved to host_pcg.h: sgx_grm_pcg_multi against sgx_grm_pcg on the golden markers, bit for bit."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.npz"))
    n, packed = 1000, g["packed"][:4000]
    rng = np.random.default_rng(9)
    mu = rng.uniform(0.02, 0.4, n)
    w = mu * (1 - mu)
    B = rng.standard_normal((7, n))
    with GrmOperator(packed, n) as op:
        for tau in ([1.0, 0.33220629], [1.0, 0.0]):
            X, its = op.pcg_many(w, tau, B, 500, 1e-5)
            for c in range(B.shape[0]):
                x1, it1 = op.pcg(w, tau, B[c], 500, 1e-5)
                assert np.array_equal(x1, X[c]) and it1 == its[c]
