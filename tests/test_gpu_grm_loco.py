"""GPU: the leave-one-group-out forms of the implicit-GRM operator (sgx_grm_set_groups, sgx_grm_diag_loco,
sgx_grm_crossprod_loco, sgx_grm_pcg_loco) against the long-double reference of grm_loco_ref.py, at the tile-edge
shapes of grm_ref.py and over group layouts whose boundaries fall inside a 16-marker dword and a 256-row tile,
interleave, leave a group empty, or leave nearly nothing.

Bounds are those of test_gpu_grm_edges.py: diag at rtol 1e-12; every product within 4 E_ORC of scaled_error
and within max|out - ref| <= 1e-11 max|ref| (the second not for the constant vector, whose max|ref| is
rounding-sized); PCG with the reference's iteration counts and rtol 1e-8, atol 1e-10 max|x|."""
import numpy as np
import pytest

import grm_loco_ref as LR
import grm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

BOUND = 4 * R.E_ORC


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def _check_products(out, ref, what):
    for j in range(out.shape[0]):
        kind = R.VECTOR_KINDS[j % len(R.VECTOR_KINDS)]
        e = R.scaled_error(out[j], ref.out[j], ref.scale[j])
        mx = float(np.max(np.abs(ref.out[j])))
        rel = float(np.max(np.abs(out[j] - ref.out[j]))) / mx if mx > 0 else float(np.max(np.abs(out[j])))
        assert e <= BOUND, (what, j, kind, e)
        if kind not in R.CONSTANT_KINDS:
            assert rel <= 1e-11, (what, j, kind, rel)


def _all_columns(B, n_groups, sizes, m):
    """Every vector against every legal excl (-1 and each group that leaves a marker) -> (B rows, excl)."""
    ex = [-1] + [c for c in range(n_groups) if sizes[c] < m]
    return np.vstack([B] * len(ex)), np.repeat(ex, B.shape[0])


# ---- a. diag and products at every shape and layout
@pytest.mark.parametrize("name", LR.LAYOUTS)
@pytest.mark.parametrize("n,m", LR.LOCO_SHAPES)
def test_diag_and_products_against_long_double(n, m, name):
    from saigegds_amd._lib import GrmOperator
    cs = R.case(n, m, 5e-3)
    group, ng = LR.layout(name, m)
    sizes = np.bincount(group, minlength=ng)
    Bk, ex = _all_columns(cs.B, ng, sizes, m)
    with GrmOperator(R.pack(cs.codes), n) as op:
        op.set_groups(group, ng)
        assert np.array_equal(op.group_sizes(), sizes)
        diags = {c: op.diag_loco(c) for c in np.unique(ex)}
        out = op.crossprod_loco(Bk, ex)
        full = op.diag()
    assert np.array_equal(diags[-1], full)
    for c, d in diags.items():
        np.testing.assert_allclose(d, LR.diag_excl(cs.codes, group, c).astype(np.float64), rtol=1e-12, atol=0, err_msg=str(c))
        if c >= 0 and sizes[c] == 0:
            assert np.array_equal(d, full)              # excluding an empty group is excluding nothing
    _check_products(out, LR.reference_loco(cs.codes, group, Bk, ex), (n, m, name))


def test_thirty_percent_missing_interleaved():
    from saigegds_amd._lib import GrmOperator
    n, m = 257, 255
    cs = R.case(n, m, 0.3)
    group, ng = LR.layout("interleaved", m)
    Bk, ex = _all_columns(cs.B, ng, np.bincount(group, minlength=ng), m)
    with GrmOperator(R.pack(cs.codes), n) as op:
        op.set_groups(group, ng)
        out = op.crossprod_loco(Bk, ex)
    _check_products(out, LR.reference_loco(cs.codes, group, Bk, ex), "miss0.3")


def test_sample_whose_remaining_codes_are_all_missing():
    from saigegds_amd._lib import GrmOperator
    n, m = 257, 255
    codes, group, ng = LR.zero_diag_case(n, m)
    B = R.case(n, m, 5e-3).B
    Bk, ex = _all_columns(B, ng, np.bincount(group, minlength=ng), m)
    with GrmOperator(R.pack(codes), n) as op:
        op.set_groups(group, ng)
        d_full, d1 = op.diag_loco(-1), op.diag_loco(1)
        out = op.crossprod_loco(Bk, ex)
    assert d_full[0] > 0 and d1[0] == 0
    np.testing.assert_allclose(d1, LR.diag_excl(codes, group, 1).astype(np.float64), rtol=1e-12, atol=0)
    finite = [j for j in range(Bk.shape[0]) if ex[j] == 1]
    assert np.all(out[finite, 0] == 0)                  # a sum of zero terms, not rounding noise (scaled_error too)
    _check_products(out, LR.reference_loco(codes, group, Bk, ex), "zero diag")


# ---- b. excl = -1 and the plain entries
def test_no_exclusion_is_the_plain_operator_bit_for_bit():
    from saigegds_amd._lib import GrmOperator
    n, m = 257, 255
    cs = R.case(n, m, 5e-3)
    pk = R.pack(cs.codes)
    _, w, Bp = R.pcg_inputs(n, m)
    rng = np.random.default_rng(5)
    B9 = np.vstack([cs.B, rng.standard_normal((2, n))])
    tau = [1.0, 0.33]
    none3, none9 = np.full(3, -1), np.full(9, -1)
    with GrmOperator(pk, n) as op:
        before = (op.diag(), op.crossprod(cs.B[0]), op.crossprod_many(B9), op.pcg(w, tau, Bp[2], R.PCG_MAXITER, R.PCG_TOL),
                  op.pcg_many(w, tau, Bp, R.PCG_MAXITER, R.PCG_TOL))
        # legal before set_groups as long as nothing is excluded
        assert np.array_equal(op.crossprod_loco(B9, none9), before[2])
        X, its = op.pcg_loco(w[None, :], np.zeros(3, dtype=int), tau, Bp, none3, R.PCG_MAXITER, R.PCG_TOL)
        assert np.array_equal(X, before[4][0]) and np.array_equal(its, before[4][1])
        op.set_groups(np.arange(m) % 3, 3)
        after = (op.diag(), op.crossprod(cs.B[0]), op.crossprod_many(B9), op.pcg(w, tau, Bp[2], R.PCG_MAXITER, R.PCG_TOL),
                 op.pcg_many(w, tau, Bp, R.PCG_MAXITER, R.PCG_TOL))
        assert np.array_equal(op.crossprod_loco(B9, none9), before[2])
        X, its = op.pcg_loco(np.vstack([w, w]), [1, 0, 1], tau, Bp, none3, R.PCG_MAXITER, R.PCG_TOL)
        assert np.array_equal(X, before[4][0]) and np.array_equal(its, before[4][1])
    assert np.all(before[4][1] > 0)
    for a, b in zip(before, after):
        if isinstance(a, tuple):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        else:
            assert np.array_equal(a, b)


# ---- c. a column's bits do not depend on its neighbours, its position or k
def test_column_independence():
    from saigegds_amd._lib import GrmOperator
    n, m = 513, 511
    cs = R.case(n, m, 5e-3)
    group, ng = LR.layout("contig", m)
    rng = np.random.default_rng(11)
    mu = rng.uniform(0.02, 0.4, (3, n))
    W = mu * (1 - mu)
    tau = [1.0, 0.33]
    b = cs.B[0]
    others = rng.standard_normal((64, n)) * 10.0 ** rng.uniform(-1, 1, (64, 1))
    with GrmOperator(R.pack(cs.codes), n) as op:
        op.set_groups(group, ng)
        for c in (2, -1):
            alone = op.crossprod_loco(b[None, :], [c])[0]
            x_alone, it_alone = op.pcg_loco(W, [1], tau, b[None, :], [c], R.PCG_MAXITER, R.PCG_TOL)
            assert it_alone[0] > 1
            # (k, position): 7 columns cross GRM_GROUP = 6 and GRM_GROUP2 = 3; 64 cross every sub-group edge
            for k, pos in ((7, 0), (7, 6), (7, 3), (64, 40), (64, 63)):
                Bk = others[:k].copy()
                Bk[pos] = b
                ex = np.arange(k) % (ng + 1) - 1
                ex[pos] = c
                wi = np.arange(k) % 3
                wi[pos] = 1
                assert np.array_equal(op.crossprod_loco(Bk, ex)[pos], alone), (c, k, pos)
                X, its = op.pcg_loco(W, wi, tau, Bk, ex, R.PCG_MAXITER, R.PCG_TOL)
                assert np.array_equal(X[pos], x_alone[0]) and its[pos] == it_alone[0], (c, k, pos)


# ---- d. against an operator built from the markers outside the group
@pytest.mark.parametrize("name", LR.LAYOUTS)
def test_against_an_operator_of_the_remaining_markers(name):
    from saigegds_amd._lib import GrmOperator
    n, m = 257, 255
    cs = R.case(n, m, 5e-3)
    group, ng = LR.layout(name, m)
    c = 0 if name == "empty" else 1
    ex = np.full(cs.B.shape[0], c)
    with GrmOperator(R.pack(cs.codes), n) as op:
        op.set_groups(group, ng)
        out, d = op.crossprod_loco(cs.B, ex), op.diag_loco(c)
    with GrmOperator(R.pack(cs.codes[group != c]), n) as sub:
        out_sub, d_sub = sub.crossprod_many(cs.B), sub.diag()
    ref = LR.reference_loco(cs.codes, group, cs.B, ex)
    _check_products(out, ref, name)
    _check_products(out_sub, ref, name + " subset")
    np.testing.assert_allclose(d, d_sub, rtol=2e-12, atol=0)      # each within 1e-12 of the reference
    assert np.array_equal(d == 0, d_sub == 0)


# ---- e. PCG with per-column weights and mixed exclusions
@pytest.mark.parametrize("n,m", R.PCG_SHAPES)
def test_pcg_loco_matches_the_numpy_pcg(n, m):
    from saigegds_amd._lib import GrmOperator
    codes, w, B = R.pcg_inputs(n, m)
    group, ng = (np.arange(m) % 3).astype(np.int32), 3
    rng = np.random.default_rng([R.PCG_SEED[(n, m)], n, 29])
    mu = rng.uniform(0.02, 0.4, (2, n))
    W = np.vstack([w, mu * (1 - mu)])
    # 9 columns: every right-hand side with every weight row, exclusions mixed over -1 .. 2
    Bk = np.vstack([B, B, B])
    wi = np.repeat([0, 1, 2], 3)
    ex = np.array([-1, 0, 1, 2, -1, 0, 1, 2, -1])
    with GrmOperator(R.pack(codes), n) as op:
        op.set_groups(group, ng)
        for tau in R.PCG_TAUS:         # [1e-6, 0]: minv at the 1e-4 clamp everywhere, and tau1 = 0
            X, its = op.pcg_loco(W, wi, tau, Bk, ex, R.PCG_MAXITER, R.PCG_TOL)
            Xr, itr = LR.pcg_reference(codes, group, W, wi, tau, Bk, ex, R.PCG_MAXITER, R.PCG_TOL)
            print(tau, "iters", its.tolist(), itr.tolist())
            assert np.array_equal(its, itr), (tau, its, itr)
            for j in range(Bk.shape[0]):
                np.testing.assert_allclose(X[j], Xr[j], rtol=1e-8, atol=1e-10 * np.max(np.abs(Xr[j])), err_msg=str((tau, j)))
        X0, its0 = op.pcg_loco(W, wi, [1.0, 0.33], Bk, ex, 0, R.PCG_TOL)
        assert np.all(its0 == 0) and np.all(X0 == 0)


# ---- f. errors: a return code and a message, nothing faults
def test_argument_errors():
    from saigegds_amd._lib import GRM_MAX_GROUPS, GrmOperator, SgxError
    n, m = 257, 255
    cs = R.case(n, m, 5e-3)
    b = cs.B[:2]
    w = np.full((1, n), 0.2)
    with GrmOperator(R.pack(cs.codes), n) as op:
        def refused(match, f):
            with pytest.raises(SgxError, match=match) as ei:
                f()
            assert ei.value.code != 0

        for f in (lambda: op.crossprod_loco(b, [-1, 0]), lambda: op.diag_loco(0), lambda: op.group_sizes(),
                  lambda: op.pcg_loco(w, [0, 0], [1.0, 0.3], b, [0, -1])):
            refused("set_groups", f)
        refused("n_groups", lambda: op.set_groups(np.zeros(m, dtype=np.int32), GRM_MAX_GROUPS + 1))
        refused("n_groups", lambda: op.set_groups(np.zeros(m, dtype=np.int32), 0))
        refused("group\\[", lambda: op.set_groups(np.where(np.arange(m) == 9, 3, 0), 3))
        refused("group\\[", lambda: op.set_groups(np.where(np.arange(m) == 9, -1, 0), 3))
        refused("set_groups", lambda: op.crossprod_loco(b, [-1, 0]))        # a refused set_groups sets nothing
        op.set_groups(np.ones(m, dtype=np.int32), 3)                       # groups 0 and 2 are empty
        refused("leaves no marker", lambda: op.crossprod_loco(b, [-1, 1]))
        refused("leaves no marker", lambda: op.diag_loco(1))
        refused("leaves no marker", lambda: op.pcg_loco(w, [0, 0], [1.0, 0.3], b, [1, -1]))
        refused("outside", lambda: op.crossprod_loco(b, [3, -1]))
        refused("excl", lambda: op.crossprod_loco(b, [-2, -1]))
        refused("w_idx", lambda: _raw_pcg(op, w, np.array([0, 1], dtype=np.int32), b))
        # the handle still works, and excluding an empty group is excluding nothing
        assert np.array_equal(op.crossprod_loco(b, [0, 2]), op.crossprod_many(b))
        op.set_groups(np.arange(m) % 2, 2)                                 # a second call replaces the first
        assert np.array_equal(op.group_sizes(), [(m + 1) // 2, m // 2])


def _raw_pcg(op, w, wi, b):
    from saigegds_amd._lib import check
    n, k = op.n, b.shape[0]
    b = np.ascontiguousarray(b)
    tau, ex = np.array([1.0, 0.3]), np.full(k, -1, dtype=np.int32)
    X, its = np.empty_like(b), np.zeros(k, dtype=np.int32)
    check(op._L.sgx_grm_pcg_loco(op._h, w.ctypes.data, n, w.shape[0], wi.ctypes.data, tau.ctypes.data, b.ctypes.data, n, k,
                                 ex.ctypes.data, 10, 1e-5, X.ctypes.data, its.ctypes.data))
