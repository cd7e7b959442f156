"""CPU: the double-precision GRM oracle (oracle/grm_oracle.c) against the long-double reference of
grm_ref.py over the whole case table -- this measures the oracle budget E_ORC that bounds the HIP
operator in test_gpu_grm_edges.py -- the packing helper against unpack_dosage_2bit, and the
conditioning of the PCG inputs that the GPU test compares iteration counts on."""
import numpy as np
import pytest

import grm_ref as R


def test_planted_features():
    """make_codes plants what its docstring says (at a shape that has room for all of it)."""
    n, m = 257, 255
    codes = R.make_codes(n, m, 1, 5e-3)
    assert codes.shape == (m, n) and codes.dtype == np.uint8 and codes.max() == 3
    miss = codes == 3
    assert np.all(miss[:, n - 1])                                   # a sample missing at every marker
    assert np.all(miss[m - 1])                                      # an all-missing marker
    assert np.all(codes[0, : n - 1] == 0)                           # a monomorphic marker
    assert 0.55 < miss[m // 2].mean() < 0.65                        # 60 % missing
    assert miss[m // 4].sum() == 1                                  # only sample n - 1 missing
    r = (3 * m) // 4
    assert np.sort(codes[r, : n - 1])[-2:].tolist() == [0, 1]       # a singleton
    af, inv = R.marker_stats(codes)
    assert af[m - 1] == 0 and inv[m - 1] == 0 and inv[0] == 0 and inv[r] > 0
    assert np.array_equal(codes, R.make_codes(n, m, 1, 5e-3))       # deterministic


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_pack_round_trip(c):
    from saigegds_amd.gds import unpack_dosage_2bit
    cs = R.case(*c)
    nb = (cs.n + 3) // 4
    plain = R.pack(cs.codes)
    assert plain.shape == (cs.m, nb)
    padded = R.pack(cs.codes, pad=0xFF)
    wide = R.pack(cs.codes, stride=nb + 37, pad=0xFF)
    assert wide.shape == (cs.m, nb + 37) and np.all(wide[:, nb:] == 0xFF)
    if cs.n % 4:
        assert np.all(padded[:, -1] >> (2 * (cs.n % 4)) == 0xFF >> (2 * (cs.n % 4)))
        assert np.all(plain[:, -1] >> (2 * (cs.n % 4)) == 0)
    for p in (plain, padded, wide):
        assert np.array_equal(unpack_dosage_2bit(p, cs.n), cs.codes)


_measured = {}


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_oracle_within_budget(c):
    from oracle import GrmOracle
    cs = R.case(*c)
    orc = GrmOracle(R.pack(cs.codes, pad=0xFF), cs.n)
    np.testing.assert_allclose(orc.diag(), cs.ref.diag.astype(np.float64), rtol=1e-12, atol=0)
    errs = [R.scaled_error(orc.crossprod(cs.B[k]), cs.ref.out[k], cs.ref.scale[k]) for k in range(len(R.VECTOR_KINDS))]
    _measured[c] = errs
    print(R.case_id(c), " ".join("%s=%.3g" % kv for kv in zip(R.VECTOR_KINDS, errs)))
    assert max(errs) <= R.E_ORC, dict(zip(R.VECTOR_KINDS, errs))


def test_oracle_budget_is_the_measured_one():
    """E_ORC is the measurement, not a guess above it: the table's worst case comes within 1 % of it."""
    if len(_measured) < len(R.CASES):
        for c in R.CASES:
            if c not in _measured:
                test_oracle_within_budget(c)
    worst = max(max(e) for e in _measured.values())
    assert 0.99 * R.E_ORC <= worst <= R.E_ORC, worst


def test_old_metric_is_blind_for_constant_vectors():
    """Why scaled_error: against max|ref| the oracle itself is off by tens of per cent for b = 1 (G 1 cancels to
    rounding level), so a bound of 1e-11 max|ref| can say nothing there; for a normal vector it reads ~1e-15."""
    from oracle import GrmOracle
    cs = R.case(20000, 40, 0.3)
    orc = GrmOracle(R.pack(cs.codes), cs.n)
    rel = {}
    for kind in ("normal", "ones"):
        k = R.VECTOR_KINDS.index(kind)
        ref = cs.ref.out[k]
        rel[kind] = float(np.max(np.abs(orc.crossprod(cs.B[k]) - ref)) / np.max(np.abs(ref)))
    assert rel["normal"] < 1e-13 and rel["ones"] > 1e-3, rel


@pytest.mark.parametrize("n,m", R.PCG_SHAPES)
def test_pcg_inputs_are_well_conditioned(n, m):
    """The GPU test requires the oracle's iteration counts.  They are only meaningful where the stopping
    test rr > tol is not decided by the last bits of rr: the oracle must stop at the same iteration with
    tol 1 % higher and 1 % lower.  A condition on the inputs (PCG_SEED), decided on the CPU alone."""
    from oracle import GrmOracle
    codes, w, B = R.pcg_inputs(n, m)
    orc = GrmOracle(R.pack(codes), n)
    assert w.min() < 0.025 and w.max() > 0.2
    for tau in R.PCG_TAUS:
        d = tau[0] / w
        if tau == [1e-6, 0.0]:
            assert np.all(d < 1e-4)
        if tau == [2e-5, 0.0]:
            assert np.any(d < 1e-4) and np.any(d > 1e-4)
        for j, name in enumerate(R.PCG_RHS):
            its = [orc.pcg(w, tau, B[j], R.PCG_MAXITER, t)[1] for t in (R.PCG_TOL, 1.01 * R.PCG_TOL, R.PCG_TOL / 1.01)]
            assert its[0] == its[1] == its[2], (tau, name, its)
            assert 0 < its[0] < R.PCG_MAXITER, (tau, name, its)
