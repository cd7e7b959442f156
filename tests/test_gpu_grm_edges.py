"""GPU: the implicit-GRM operator (kern_grm.h, host_grm.h, grm_contract_kernel<NBFV>) against the
long-double reference of grm_ref.py at the tile edges of its kernels (256-row workgroups, pairs of
256-sample tiles, the 64 x 256 transpose tile, 16-marker dwords), with N and M in both roles, at 0.5 %
and 30 % missing, for constant, wide-range and extreme-scale vectors; stray codes in the padding; the
device entry points and leading dimensions; one handle across calls of different widths; and PCG at the
preconditioner clamp.

Accuracy bound.  scaled_error (grm_ref.py) of every product is at most 4 E_ORC, E_ORC being the worst
scaled error of the double-precision oracle over the same table (test_grm_ref.py).  The kernel's
fma(code, inv, l0) adds one rounding per entry, of the kind of the oracle's rounded table; the limb
quantisation is below the rounding of a double dot product (mf_fixed.h); 4 covers the different
summation order and the ~10 double operations of the two epilogues."""
import numpy as np
import pytest

import grm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

BOUND = 4 * R.E_ORC
SENTINEL = -7.25e77


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


_worst = {}


# ---- a. accuracy at every shape
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_accuracy_against_long_double(c):
    from saigegds_amd._lib import GrmOperator
    cs = R.case(*c)
    assert cs.n * cs.m <= 800_000
    with GrmOperator(R.pack(cs.codes), cs.n) as op:
        diag = op.diag()
        outs = [op.crossprod(cs.B[k]) for k in range(len(R.VECTOR_KINDS))]
    np.testing.assert_allclose(diag, cs.ref.diag.astype(np.float64), rtol=1e-12, atol=0)
    errs, rels = [], []
    for k, kind in enumerate(R.VECTOR_KINDS):
        errs.append(R.scaled_error(outs[k], cs.ref.out[k], cs.ref.scale[k]))
        mx = float(np.max(np.abs(cs.ref.out[k])))
        rels.append(float(np.max(np.abs(outs[k] - cs.ref.out[k]))) / mx if mx > 0 else float(np.max(np.abs(outs[k]))))
        _worst[kind] = max(_worst.get(kind, 0.0), errs[-1])
    print("\n" + R.case_id(c), "scaled:", " ".join("%s=%.3g" % kv for kv in zip(R.VECTOR_KINDS, errs)))
    print(R.case_id(c), "rel:", " ".join("%s=%.2g" % kv for kv in zip(R.VECTOR_KINDS, rels)))
    print("worst so far:", " ".join("%s=%.3g" % kv for kv in _worst.items()))
    for kind, e, rel in zip(R.VECTOR_KINDS, errs, rels):
        assert e <= BOUND, (kind, e)
        if kind not in R.CONSTANT_KINDS:
            assert rel <= 1e-11, (kind, rel)       # the project's bound, max|out - ref| <= 1e-11 max|ref|


# ---- b. padding and stride
@pytest.mark.parametrize("n,m", [(17, 65), (255, 257), (513, 511), (1025, 33)])
def test_padding_codes_and_stride_do_not_count(n, m):
    from saigegds_amd._lib import GrmOperator, geno_stats_2bit
    cs = R.case(n, m, 5e-3)
    nb = (n + 3) // 4
    packs = [R.pack(cs.codes), R.pack(cs.codes, pad=0xFF), R.pack(cs.codes, stride=nb + 37, pad=0xFF)]
    assert packs[2].shape[1] % 4 != 0
    kinds = [R.VECTOR_KINDS.index(k) for k in ("normal", "ones", "wide")]
    res = []
    for p in packs:
        with GrmOperator(p, n) as op:
            res.append((op.diag(), [op.crossprod(cs.B[k]) for k in kinds], op.crossprod_many(cs.B)))
    valid = cs.codes != 3
    nv_ref, sm_ref = valid.sum(axis=1), np.where(valid, cs.codes, 0).sum(axis=1, dtype=np.int64)
    for j, p in enumerate(packs):
        nv, sm = geno_stats_2bit(p, n)
        assert np.array_equal(nv, nv_ref) and np.array_equal(sm, sm_ref), j
    np.testing.assert_allclose(res[0][0], cs.ref.diag.astype(np.float64), rtol=1e-12, atol=0)
    for j in (1, 2):
        assert np.array_equal(res[j][0], res[0][0]), j
        for a, b in zip(res[j][1], res[0][1]):
            assert np.array_equal(a, b), j
        assert np.array_equal(res[j][2], res[0][2]), j
    for k in range(len(R.VECTOR_KINDS)):
        assert R.scaled_error(res[0][2][k], cs.ref.out[k], cs.ref.scale[k]) <= BOUND, k


# ---- c. device entry points and leading dimensions
@pytest.mark.parametrize("n,m", [(513, 511), (20000, 40)])
def test_device_entry_points(n, m):
    import torch
    from saigegds_amd._lib import GrmOperator, check
    cs = R.case(n, m, 5e-3)
    pk = R.pack(cs.codes)
    dev = torch.device("cuda:0")
    k, ldb = len(R.VECTOR_KINDS), n + 5
    assert k == 7
    with GrmOperator(pk, n) as op:
        diag = op.diag()
        singles = [op.crossprod(cs.B[j]) for j in range(k)]
        # the host form with a leading dimension: gaps of B are not read (NaN there), gaps of Out not written
        Bh = np.full((k, ldb), np.nan)
        Bh[:, :n] = cs.B
        Oh = np.full((k, ldb), SENTINEL)
        check(op._L.sgx_grm_crossprod_multi(op._h, Bh.ctypes.data, ldb, k, Oh.ctypes.data))
        for j in range(k):
            assert np.array_equal(Oh[j, :n], singles[j]), j
        assert np.all(Oh[:, n:] == SENTINEL)
    for j in range(k):
        assert R.scaled_error(singles[j], cs.ref.out[j], cs.ref.scale[j]) <= BOUND, j
    pk_t = torch.from_numpy(pk).to(dev)
    B_t = torch.from_numpy(Bh).to(dev)
    O_t = torch.full((k, ldb), SENTINEL, dtype=torch.float64, device=dev)
    b_t = torch.from_numpy(np.ascontiguousarray(cs.B[0])).to(dev)
    o_t = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with GrmOperator(None, n, dev_ptr=pk_t.data_ptr(), n_markers=m, bytes_per_marker=pk.shape[1]) as opd:
        assert np.array_equal(opd.diag(), diag)
        opd.crossprod_dev(b_t.data_ptr(), o_t.data_ptr())
        opd.sync()
        assert np.array_equal(o_t.cpu().numpy(), singles[0])
        opd.crossprod_many_dev(B_t.data_ptr(), ldb, k, O_t.data_ptr())
        opd.sync()
        Od = O_t.cpu().numpy()
        for j in range(k):
            assert np.array_equal(Od[j, :n], singles[j]), j
        assert np.all(Od[:, n:] == SENTINEL)
        assert np.array_equal(pk_t.cpu().numpy(), pk)          # the caller's matrix is copied, not touched


# ---- d. one handle, many calls
def test_one_handle_across_calls_of_different_widths():
    from saigegds_amd._lib import GrmOperator
    n, m = 257, 255
    cs = R.case(n, m, 5e-3)
    pk = R.pack(cs.codes)
    _, w, Bp = R.pcg_inputs(n, m)
    rng = np.random.default_rng(41)
    tau = [1.0, 0.33]
    Bk = {k: rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-3, 3, (k, 1)) for k in (33, 1, 6, 2, 9, 3)}
    b0 = rng.standard_normal(n)
    bnan = rng.standard_normal(n)
    bnan[n // 3] = np.nan
    steps = [
        ("many33", lambda op: op.crossprod_many(Bk[33])),
        ("many1", lambda op: op.crossprod_many(Bk[1])),
        ("many6", lambda op: op.crossprod_many(Bk[6])),
        ("many2", lambda op: op.crossprod_many(Bk[2])),
        ("normal", lambda op: op.crossprod(b0)),
        ("zero", lambda op: op.crossprod(np.zeros(n))),
        ("nan", lambda op: op.crossprod(bnan)),
        ("normal again", lambda op: op.crossprod(b0)),
        ("pcg_many9", lambda op: op.pcg_many(w, tau, np.vstack([Bp, Bk[6]]), R.PCG_MAXITER, R.PCG_TOL)),
        ("pcg", lambda op: op.pcg(w, tau, Bp[2], R.PCG_MAXITER, R.PCG_TOL)),
        ("many3", lambda op: op.crossprod_many(Bk[3])),
    ]

    def parts(r):
        return [np.asarray(a) for a in r] if isinstance(r, tuple) else [r]

    with GrmOperator(pk, n) as op:
        reused = [(name, f(op)) for name, f in steps]
    got = dict(reused)
    assert np.all(got["zero"] == 0)
    assert np.all(np.isnan(got["nan"]))                     # as the reference's loop: every dot product is NaN
    assert np.array_equal(got["normal"], got["normal again"])
    assert np.all(got["pcg_many9"][1] > 0) and got["pcg"][1] == got["pcg_many9"][1][2]
    for (name, f), (_, r) in zip(steps, reused):
        with GrmOperator(pk, n) as fresh:
            want = f(fresh)
        for a, b in zip(parts(r), parts(want)):
            assert np.array_equal(a, b, equal_nan=True), name


# ---- e. PCG, the preconditioner clamp included
@pytest.mark.parametrize("n,m", R.PCG_SHAPES)
def test_pcg_matches_oracle_at_the_clamp(n, m):
    from oracle import GrmOracle
    from saigegds_amd._lib import GrmOperator
    codes, w, B = R.pcg_inputs(n, m)
    pk = R.pack(codes)
    orc = GrmOracle(pk, n)
    with GrmOperator(pk, n) as op:
        for tau in R.PCG_TAUS:
            X, its = op.pcg_many(w, tau, B, R.PCG_MAXITER, R.PCG_TOL)
            for j, name in enumerate(R.PCG_RHS):
                xr, itr = orc.pcg(w, tau, B[j], R.PCG_MAXITER, R.PCG_TOL)
                xg, itg = op.pcg(w, tau, B[j], R.PCG_MAXITER, R.PCG_TOL)
                print(tau, name, "iters", itg, itr)
                assert itg == itr, (tau, name, itg, itr)     # conditioned by test_pcg_inputs_are_well_conditioned
                np.testing.assert_allclose(xg, xr, rtol=1e-8, atol=1e-10 * np.max(np.abs(xr)), err_msg=str((tau, name)))
                assert its[j] == itg and np.array_equal(X[j], xg), (tau, name)
        x0, it0 = op.pcg(w, [1.0, 0.33], B[0], 0, R.PCG_TOL)
        assert it0 == 0 and np.all(x0 == 0)
        X0, its0 = op.pcg_many(w, [1.0, 0.33], B, 0, R.PCG_TOL)
        assert np.all(its0 == 0) and np.all(X0 == 0)
