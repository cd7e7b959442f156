"""GPU: the tall-skinny FP64 block kernels of the GRM's principal components (kern_tsblock.h: ts_gram on the FP64 matrix
cores, ts_apply) against np.longdouble at the edges of their tiles -- 16 columns a fragment, 4 rows an MFMA step, 32 rows
a staging step, SGX_TS_SLAB rows a partial -- and the marker side of the operator's product (sgx_grm_marker_dots).

Bounds.  |C_ab - ref| <= N 2^-53 sum_i |A_ia| |B_ib| holds for any order of an N-term sum of exact products (the
matrix cores fuse each product into the sum); |Out_ic - ref| <= L 2^-53 sum_a |A_ia| |T_ac| for a chain of L fused
multiply-adds.  marker_dots: dot_v = l0_v (sum b - sum_missing b) + inv_v sum code b is measured, as grm_ref.py
measures the product, against the sum of the magnitudes of its terms,
scale_v = (|l0_v| (N + n_missing_v) + inv_v sum_i code_vi) max|b|, in units of 2^-53, and held to the product's own
bound 4 E_ORC: it is the first half of that product (the exact integer sums, one rounded sum of b, the same
three-operation expression)."""
import functools

import numpy as np
import pytest

import grm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

LD = np.longdouble
U = 2.0 ** -53
BOUND_DOTS = 4 * R.E_ORC
SENTINEL = -7.25e77
LS = (1, 2, 15, 16, 17, 33, 64)


def _slab():
    from saigegds_amd._lib import TS_SLAB
    return TS_SLAB


def _ns():
    s = _slab()
    return (1, 3, 4, 5, 63, 64, 65, s - 1, s, s + 1, 2 * s + 7)


@pytest.fixture(scope="module")
def op():
    import torch
    assert torch.cuda.is_available()
    from saigegds_amd._lib import GrmOperator
    codes = R.make_codes(5, 3, 1, 5e-3)
    with GrmOperator(R.pack(codes), 5) as o:
        yield o


@functools.lru_cache(maxsize=None)
def blocks(n):
    """A [64, ld], B [33, ld] with ld = n + 5 and NaN in rows n .. ld - 1; read-only."""
    rng = np.random.default_rng([n, 41])
    ld = n + 5
    A = rng.standard_normal((64, ld)) * 10.0 ** rng.uniform(-2, 2, (64, 1))
    B = rng.standard_normal((33, ld))
    A[:, n:] = np.nan
    B[:, n:] = np.nan
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def _gram_ref(A, B, n):
    a, b = A[:, :n].astype(LD), B[:, :n].astype(LD)
    return a @ b.T, n * U * (np.abs(a) @ np.abs(b).T)


def _worst(C, ref, bound):
    assert np.isfinite(C).all()
    err = np.abs(C.astype(LD) - ref)
    assert (err <= bound).all(), float(np.max(err / np.where(bound > 0, bound, 1)))
    return float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("n", _ns())
def test_gram_against_long_double(op, n):
    A, B = blocks(n)
    full = op.ts_gram(A, n=n)
    worst = 0.0
    for L in LS:
        C = op.ts_gram(A[:L], n=n)
        assert C.shape == (L, L)
        ref, bound = _gram_ref(A[:L], A[:L], n)
        worst = max(worst, _worst(C, ref, bound))
        np.testing.assert_array_equal(C, C.T)                          # the same two columns either way round
        np.testing.assert_array_equal(C, full[:L, :L])                 # the bits do not depend on L
        np.testing.assert_array_equal(C, op.ts_gram(A[:L], n=n))       # nor on the call
        np.testing.assert_array_equal(C, op.ts_gram(A[:L], A[:L].copy(), n=n))   # nor on B being A itself
    for La, Lb in ((17, 33), (64, 1), (2, 15), (33, 16)):
        C = op.ts_gram(A[:La], B[:Lb], n=n)
        assert C.shape == (La, Lb)
        ref, bound = _gram_ref(A[:La], B[:Lb], n)
        worst = max(worst, _worst(C, ref, bound))
        np.testing.assert_array_equal(C, op.ts_gram(B[:Lb], A[:La], n=n).T)
    print(f"\nts_gram n={n}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("n", (5, 65, _slab() + 1, 2 * _slab() + 7))
def test_gram_bits_do_not_depend_on_position_or_neighbours(op, n):
    A, B = blocks(n)
    full = op.ts_gram(A, n=n)
    rng = np.random.default_rng(n)
    for L in (2, 17, 33, 64):
        pick = rng.permutation(64)[:L]
        C = op.ts_gram(np.ascontiguousarray(A[pick]), n=n)
        np.testing.assert_array_equal(C, full[np.ix_(pick, pick)])
    # other neighbours, another stride: columns 3 and 40 of A between columns of B
    ld2 = n + 11
    mix = np.full((20, ld2), np.nan)
    mix[:, :n] = B[:20, :n]
    mix[4, :n], mix[18, :n] = A[3, :n], A[40, :n]
    C = op.ts_gram(mix, n=n)
    assert C[4, 18] == full[3, 40] and C[18, 4] == full[40, 3] and C[4, 4] == full[3, 3]
    cross = op.ts_gram(A, B, n=n)
    assert C[4, 0] == cross[3, 0] and C[18, 19] == cross[40, 19]


@pytest.mark.parametrize("n", _ns())
def test_apply_against_long_double(op, n):
    A, _ = blocks(n)
    rng = np.random.default_rng([n, 43])
    worst = 0.0
    for La, Lc in ((1, 1), (2, 17), (15, 16), (16, 15), (17, 2), (33, 64), (64, 33), (64, 64)):
        T = rng.standard_normal((La, Lc))
        out = op.ts_apply(A[:La], T, n=n, fill=SENTINEL)
        assert out.shape == (Lc, n + 5)
        np.testing.assert_array_equal(out[:, n:], SENTINEL)            # rows >= n are not written
        a = A[:La, :n].astype(LD)
        ref, bound = T.T.astype(LD) @ a, La * U * (np.abs(T.T).astype(LD) @ np.abs(a))
        worst = max(worst, _worst(out[:, :n], ref, bound))
        np.testing.assert_array_equal(out, op.ts_apply(A[:La], T, n=n, fill=SENTINEL))
        # element (i, c) depends on row i of A and column c of T only: fewer, reordered columns of T
        pick = rng.permutation(Lc)[:max(1, Lc // 2)]
        sub = op.ts_apply(A[:La], np.ascontiguousarray(T[:, pick]), n=n, fill=SENTINEL)
        np.testing.assert_array_equal(sub, out[pick])
    print(f"\nts_apply n={n}: worst error / bound = {worst:.3g}")


def test_apply_upper_triangular_leaves_leading_columns(op):
    """Q R^-1 with R^-1 upper triangular: column 0 is a multiple of column 0 of A, whatever follows it."""
    n = 65
    A, _ = blocks(n)
    T = np.triu(np.random.default_rng(5).standard_normal((16, 16)))
    out = op.ts_apply(A[:16], T, n=n)
    np.testing.assert_array_equal(out[0, :n], A[0, :n] * T[0, 0])


def test_argument_checks(op):
    from saigegds_amd._lib import SgxError
    A = np.zeros((2, 8))
    for call in (lambda: op.ts_gram(A, n=9), lambda: op.ts_gram(A, n=0), lambda: op.ts_gram(np.zeros((65, 8))),
                 lambda: op.ts_apply(A, np.zeros((2, 65))), lambda: op.ts_apply(A, np.zeros((2, 2)), n=9)):
        with pytest.raises(SgxError) as e:
            call()
        assert e.value.code == -1


# ---- the marker side of the product
@functools.lru_cache(maxsize=None)
def dots_ref(c):
    cs = R.case(*c)
    codes = cs.codes
    af, inv = R.marker_stats(codes)
    valid = codes != 3
    g = np.where(valid, (codes.astype(LD) - 2 * af.astype(LD)[:, None]) * inv.astype(LD)[:, None], LD(0))
    ref = (g @ cs.B.T.astype(LD)).T                                    # [kinds, m]
    n_miss = (~valid).sum(axis=1)
    amp = (np.abs(-2 * af * inv) * (cs.n + n_miss) + inv * np.where(valid, codes, 0).sum(axis=1)).astype(LD)
    scale = amp[None, :] * np.max(np.abs(cs.B), axis=1).astype(LD)[:, None]
    return ref, scale


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_marker_dots_against_long_double(c):
    from saigegds_amd._lib import GrmOperator
    cs = R.case(*c)
    ref, scale = dots_ref(c)
    with GrmOperator(R.pack(cs.codes), cs.n) as o:
        before = o.crossprod_many(cs.B)
        dots = o.marker_dots(cs.B)
        again = o.marker_dots(cs.B[::-1])[::-1]                        # other groups, other places in them
        after = o.crossprod_many(cs.B)
        one = o.marker_dots(cs.B[3:4])
    assert dots.shape == (len(R.VECTOR_KINDS), cs.m)
    np.testing.assert_array_equal(before, after)                       # the product is as it was, bit for bit
    np.testing.assert_array_equal(dots, again)
    np.testing.assert_array_equal(dots[3:4], one)
    errs = [R.scaled_error(dots[k], ref[k], scale[k]) for k in range(len(R.VECTOR_KINDS))]
    print("\n" + R.case_id(c), "scaled:", " ".join("%s=%.3g" % kv for kv in zip(R.VECTOR_KINDS, errs)))
    for kind, e in zip(R.VECTOR_KINDS, errs):
        assert e <= BOUND_DOTS, (kind, e)


def test_marker_dots_rebuild_the_product():
    """K b = G' dot / M: the dots are what the product's second half sums."""
    from saigegds_amd._lib import GrmOperator
    cs = R.case(257, 255, 5e-3)
    af, inv = R.marker_stats(cs.codes)
    g = np.where(cs.codes != 3, (cs.codes.astype(np.float64) - 2 * af[:, None]) * inv[:, None], 0.0)
    with GrmOperator(R.pack(cs.codes), cs.n) as o:
        dots = o.marker_dots(cs.B[:1])
        out = o.crossprod(cs.B[0])
        taf, tinv = o.marker_table()
    np.testing.assert_array_equal(taf, af)
    np.testing.assert_array_equal(tinv, inv)
    np.testing.assert_allclose(g.T @ dots[0] / cs.m, out, rtol=0, atol=1e-11 * np.abs(out).max())


def test_marker_dots_argument_checks():
    from saigegds_amd._lib import GrmOperator, SgxError, load
    cs = R.case(17, 65, 5e-3)
    with GrmOperator(R.pack(cs.codes), cs.n) as o:
        L = load()
        B = np.zeros((2, cs.n))
        out = np.zeros((2, cs.m))
        assert L.sgx_grm_marker_dots(o._h, B.ctypes.data, cs.n, 2, out.ctypes.data, cs.m - 1) == -1
        assert L.sgx_grm_marker_dots(o._h, B.ctypes.data, cs.n - 1, 2, out.ctypes.data, cs.m) == -1
        assert L.sgx_grm_marker_dots(o._h, B.ctypes.data, cs.n, 0, out.ctypes.data, cs.m) == -1
        assert L.sgx_grm_marker_dots(o._h, None, cs.n, 2, out.ctypes.data, cs.m) == -1
        with pytest.raises(ValueError):
            o.marker_dots(np.zeros((2, cs.n + 1)))
        assert SgxError is not None
