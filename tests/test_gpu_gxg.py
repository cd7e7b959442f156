"""GPU: the multi-vector GRM operator (sgx_grm_crossprod_multi / sgx_grm_pcg_multi) against the single
calls, bit for bit, and seqGLMM_GxG_spa end to end against the CPU oracle and an unbatched GPU run."""
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu]

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def _case(n, m, seed, miss=5e-3):
    from saigegds_amd import synth
    thr = synth.variant_thresholds(0, m, seed, log10_maf=(-2.0, -0.3), flip_frac=0.2, miss_rate=miss)
    packed = synth.synth_packed(n, 0, m, seed, thr)
    packed[3] = 0                      # a monomorphic marker
    packed[7, : (n + 3) // 4] = 0xFF   # an all-missing marker
    if n % 4:
        packed[:, (n + 3) // 4 - 1] &= (1 << (2 * (n % 4))) - 1
    return packed


def _rhs(n, k, rng):
    """+-1 vectors, scaled normals (1e-6 .. 3e7) and an all-zero column."""
    B = np.empty((k, n))
    for j in range(k):
        if j % 3 == 0:
            B[j] = 2.0 * rng.integers(0, 2, n) - 1
        else:
            B[j] = rng.standard_normal(n) * (1e-6 if j % 3 == 1 else 3e7) * (1 + j)
    if k > 1:
        B[k // 2] = 0
    return B


@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("n,m", [(1000, 3000), (3001, 1111), (777, 260)])
def test_crossprod_many_bit_identical(n, m):
    from oracle import GrmOracle
    from saigegds_amd._lib import GrmOperator
    packed = _case(n, m, seed=n + 7 * m)
    orc = GrmOracle(packed, n)
    rng = np.random.default_rng(n)
    with GrmOperator(packed, n) as op:
        for k in (1, 3, 8, 33):
            B = _rhs(n, k, rng)
            out = op.crossprod_many(B)
            assert out.shape == (k, n)
            for j in range(k):
                single = op.crossprod(B[j])
                assert np.array_equal(out[j], single), (k, j)
                ref = orc.crossprod(B[j])
                assert np.max(np.abs(out[j] - ref)) <= 1e-11 * max(np.max(np.abs(ref)), 1e-300), (k, j)
        # the [k, N] layout: rows are vectors; a transposed array is rejected
        with pytest.raises(ValueError):
            op.crossprod_many(np.zeros((n, 2)) if n != 2 else np.zeros((3, 3)))


@pytest.mark.timeout(600, method="thread")
def test_pcg_many_matches_single_solves():
    from saigegds_amd._lib import GrmOperator
    n, m = 1000, 3000
    packed = _case(n, m, seed=11)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.05, 0.25, n)
    k = 9
    B = _rhs(n, k, rng)
    B[1] = 5e-5 * (2.0 * rng.integers(0, 2, n) - 1)     # rr = 2.5e-6 <= tol: converged at iteration 0
    with GrmOperator(packed, n) as op:
        for tau, maxiter, tol in (((1.0, 0.5), 500, 1e-5), ((1.0, 0.0), 500, 1e-5), ((1.0, 0.3), 4, 1e-12)):
            X, iters = op.pcg_many(w, tau, B, maxiter, tol)
            if tol == 1e-5:
                assert iters[1] == 0 and np.all(X[1] == 0)
            for j in range(k):
                x, it = op.pcg(w, tau, B[j], maxiter, tol)
                assert iters[j] == it, (tau, maxiter, j)
                assert np.array_equal(X[j], x), (tau, maxiter, j)
            if maxiter == 4:
                assert np.max(iters) == 4           # the cap stops the columns that have not converged
        # more columns than one call takes: batches of SGX_GRM_MAX_RHS
        B2 = np.vstack([B] * 8)[:70]
        X2, it2 = op.pcg_many(w, (1.0, 0.5), B2, 500, 1e-5)
        X1, it1 = op.pcg_many(w, (1.0, 0.5), B, 500, 1e-5)
        assert np.array_equal(X2[:k], X1) and np.array_equal(it2[:k], it1)
        assert np.array_equal(X2[63], X1[63 % k])


@pytest.mark.timeout(600, method="thread")
def test_multi_entry_points_reject_bad_arguments():
    from saigegds_amd._lib import GrmOperator, SgxError, check
    n = 777
    packed = _case(n, 260, seed=5)
    with GrmOperator(packed, n) as op:
        L, h = op._L, op._h
        B = np.zeros((65, n))
        out = np.empty_like(B)
        it = np.zeros(65, dtype=np.int32)
        w, tau = np.ones(n), np.array([1.0, 0.5])
        for rc in (L.sgx_grm_crossprod_multi(h, B.ctypes.data, n, 65, out.ctypes.data),
                   L.sgx_grm_crossprod_multi(h, B.ctypes.data, n - 1, 2, out.ctypes.data),
                   L.sgx_grm_crossprod_multi(h, None, n, 2, out.ctypes.data),
                   L.sgx_grm_crossprod_multi_dev(h, B.ctypes.data, n, 0, out.ctypes.data),
                   L.sgx_grm_pcg_multi(h, w.ctypes.data, tau.ctypes.data, B.ctypes.data, n, 65, 10, 1e-5,
                                       out.ctypes.data, it.ctypes.data),
                   L.sgx_grm_pcg_multi(h, None, tau.ctypes.data, B.ctypes.data, n, 2, 10, 1e-5,
                                       out.ctypes.data, it.ctypes.data)):
            assert rc == -1
            with pytest.raises(SgxError):
                check(rc)


@pytest.mark.timeout(120, method="thread")
def test_short_weights_are_refused_and_handles_close_once():
    """A weight vector that is not one entry per sample never reaches the library (it reads N doubles from it), the
    operator goes on working, and every handle class frees its object once: on the first close() or on leaving ``with``."""
    from conftest import scan_model
    from saigegds_amd._lib import Block, DosageBlock, ExplicitGrmOperator, GrmOperator, Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 5, 8
    rng = np.random.default_rng(58)
    packed = pack_dosage_2bit(rng.integers(0, 3, (m, n)).astype(np.uint8))
    w, tau = rng.uniform(0.05, 0.25, n), (1.0, 0.5)
    B = np.vstack([2.0 * rng.integers(0, 2, (2, n)) - 1, rng.standard_normal((1, n))])
    with GrmOperator(packed, n) as op:
        op.set_groups(np.arange(m) % 2, 2)
        for bad in (4, 6):
            with pytest.raises(ValueError):
                op.pcg(np.ones(bad), tau, B[0])
            with pytest.raises(ValueError):
                op.pcg_many(np.ones(bad), tau, B)
            with pytest.raises(ValueError):
                op.pcg_loco(np.ones((2, bad)), [0, 1, 0], tau, B, [-1, 0, 1])
        X, its = op.pcg_many(w, tau, B)
        for j in range(len(B)):
            x, it = op.pcg(w, tau, B[j])
            assert np.array_equal(X[j], x) and its[j] == it, j
        Xl, itl = op.pcg_loco(w[None, :], [0, 0, 0], tau, B, [-1, -1, -1])
        assert np.array_equal(Xl, X) and np.array_equal(itl, its)

    sm = scan_model("saige_model.npz")
    sc = Scanner(sm)
    made = [lambda: Scanner(sm), lambda: Block(sm.n, 1), lambda: DosageBlock(sc, np.uint8, 1),
            lambda: GrmOperator(packed, n), lambda: ExplicitGrmOperator(np.eye(n))]
    for make in made:
        obj = make()
        assert getattr(obj, obj._attr)
        obj.close()
        assert getattr(obj, obj._attr) is None
        obj.close()
        assert getattr(obj, obj._attr) is None
        with make() as obj:
            assert getattr(obj, obj._attr)
        assert getattr(obj, obj._attr) is None
    sc.close()


def _man_example(**kw):
    from saigegds_amd.gxg import seqGLMM_GxG_spa
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    data = {"sample.id": ph["sample_id"], "y": ph["y"], "x1": ph["x1"], "x2": ph["x2"]}
    snp_pair = {"s1": np.array([2, 3]), "s2": np.array([6, 7]), "note": np.array(["F1", "F2"])}
    fn = os.path.join(GOLD, "grm1k_10k_snp.gds")
    return seqGLMM_GxG_spa("y ~ x1 + x2", data, fn, fn, snp_pair, trait_type="binary", verbose_detail=False,
                           verbose=False, **kw)


@pytest.mark.timeout(1800, method="thread")
def test_gxg_man_example_gpu_vs_oracle_and_unbatched():
    from oracle import GrmOracle
    gpu = _man_example()
    assert list(gpu)[:13] == ["id1", "snp1", "maf1", "id2", "snp2", "maf2", "beta", "SE", "n_nonzero", "pval",
                              "p.norm", "converged", "tau_G"]
    assert list(gpu)[13:] == ["note"]
    assert gpu["id1"].tolist() == [2, 3] and gpu["id2"].tolist() == [6, 7]
    assert gpu["snp1"].tolist() == ["1:2_1_2", "1:3_1_2"]
    assert np.all(np.isfinite(gpu["pval"])) and np.all(gpu["SE"] > 0)
    orc = _man_example(operator_factory=lambda p, n: GrmOracle(p, n))
    for k in ("id1", "snp1", "id2", "snp2", "n_nonzero", "converged", "note"):
        assert gpu[k].tolist() == orc[k].tolist(), k
    for k in ("maf1", "maf2", "beta", "SE", "pval", "tau_G"):
        np.testing.assert_allclose(gpu[k], orc[k], rtol=1e-8, atol=0, err_msg=k)
    single = _man_example(batch_solves=False)
    for k in gpu:
        assert np.array_equal(np.asarray(gpu[k]), np.asarray(single[k])), k
