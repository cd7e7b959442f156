"""sgx_ds_block_skat_kmat, sgx_ds_block_cond_kmat_set and sgx_ds_block_cond_kmat on the device, through
the ctypes binding.  The references, the case table and the recorded tolerances are in tests/kmat_ds_ref.py.

* Phi^K against the long-double reference at tol = 1e-12, maxiter = 500, scaled by sqrt(Phi_ee Phi_ff), within
  skat_kmat_ref.PHI_TOL = 5.55e-7; scores within the scan's 1e-10 rule (conftest REL_TOL / Z_FLOOR).
* hard calls loaded into a uint8, a float64 and an int32 block against the 2-bit entries on the packed form of the same
  rows: bit for bit -- the test that pins the summation order of the one-pass column kernel.
* the identity of 8h on dosages, determinism and independence, tau[1] = 0, bad entries and argument errors.
"""
import numpy as np
import pytest

import kmat_ds_ref as KD
import skat_kmat_ref as M

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in KD.CASES]


def operator(c):
    from saigegds_amd._lib import ExplicitGrmOperator
    return ExplicitGrmOperator(csr=c["csr"]) if c["storage"] == "csr" else ExplicitGrmOperator(c["K"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_units(a, b):
    return same_bits(a[0], b[0]) and len(a[1]) == len(b[1]) and all(same_bits(x, y) for x, y in zip(a[1], b[1])) \
        and np.array_equal(a[2], b[2])


def same_rows(a, b):
    return all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])


class Dev:
    """A scanner, the operator of a case and a dosage block of its dtype, open for one test."""

    def __init__(self, c, dtype=None, cap=None):
        import torch  # noqa: F401
        from saigegds_amd._lib import Scanner
        self.c = c
        self.sc = Scanner(c["sm"])
        self.op = operator(c)
        self.blk = self.sc.dosage_block(c["dtype"] if dtype is None else dtype, cap or max(1, len(c.get("rows", [0]))))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.blk.close()
        self.op.close()
        self.sc.close()

    def skat(self, unit_ptr, var_idx, flip, mean, tau=None, w=None, tol=KD.TOL_SOLVE):
        c = self.c
        return self.blk.skat_kmat(self.op, unit_ptr, var_idx, flip, mean, c["w"] if w is None else w,
                                  c["tau"] if tau is None else tau, maxiter=KD.MAXITER, tol=tol)

    def cond_set(self, var_idx, flip, mean, tau=None, w=None, tol=KD.TOL_SOLVE):
        c = self.c
        return self.blk.cond_kmat_set(self.op, var_idx, flip, mean, c["w"] if w is None else w,
                                      c["tau"] if tau is None else tau, maxiter=KD.MAXITER, tol=tol)

    def cond(self, flip, mean):
        return self.blk.cond_kmat(self.op, flip, mean)


@pytest.mark.parametrize("name", NAMES)
def test_1_against_the_long_double_reference(name):
    from conftest import REL_TOL, Z_FLOOR
    c = KD.make_case(name)
    ref = KD.case_ref(name, "ld")
    C, rows, flip, mean, up = c["n_cond"], c["rows"], c["flip"], c["mean"], c["unit_ptr"]
    with Dev(c) as d:
        d.blk.load(rows)
        score, covs, iters = d.skat(up, c["var_idx"], flip, mean)
        plain, _ = d.blk.skat(up, c["var_idx"], flip, np.where(np.isfinite(mean), mean, 0.0))
        d.blk.load(rows[:C])
        S_C, phi_cc, it_c = d.cond_set(np.arange(C), flip[:C], mean[:C])
        d.blk.load(rows[C:])
        S, var, cov, it = d.cond(flip[C:], mean[C:])
    bad = ~np.isfinite(mean)
    assert int(max(iters.max(), it.max(), it_c.max())) < KD.MAXITER and np.all(iters[bad] == 0)
    # scores: the scan's rule, against the long-double reference and against sgx_ds_block_skat's own
    S_ref = np.asarray(ref["S"], dtype=np.float64)
    sd = np.sqrt(np.maximum(np.concatenate([np.diag(np.asarray(p, dtype=np.float64)) for p in ref["skat"]]), 0))
    ok = ~bad
    assert np.array_equal(np.isnan(score), bad)
    e_s = np.abs(score[ok] - S_ref[ok]) - (REL_TOL * np.abs(S_ref[ok]) + Z_FLOOR * np.nan_to_num(sd[ok]) + 1e-300)
    assert float(e_s.max()) <= 0, f"{name}: score off the reference by {float(np.abs(score[ok] - S_ref[ok]).max()):.3g}"
    assert np.all(np.abs(score[ok] - plain[ok]) <= REL_TOL * np.abs(plain[ok]) + 1e-9 * np.abs(S_ref[ok]).max())
    assert same_bits(np.concatenate([S_C, S]), score[np.arange(len(rows))])         # one column kernel for all three
    worst = 0.0
    for u, (p, r) in enumerate(zip(covs, ref["skat"])):
        assert np.array_equal(p, p.T, equal_nan=True), f"{name} unit {u}"
        if p.size:
            worst = max(worst, KD.finite_error(p, r))
    worst = max(worst, KD.finite_error(phi_cc, ref["Phi_CC"]))
    for j, r in enumerate(ref["units"]):
        u = np.empty((C + 1, C + 1))
        u[:C, :C], u[C, :C], u[:C, C], u[C, C] = phi_cc, cov[j], cov[j], var[j]
        worst = max(worst, KD.finite_error(u, r))
    print(f"{name}: Phi^K off the long-double reference by {worst:.3g} (bound {M.PHI_TOL:.3g}), iters <= "
          f"{int(max(iters.max(), it.max()))}")
    assert worst <= M.PHI_TOL, name


def hard_case(n, kcov):
    """Hard calls for the bit-for-bit test: 7 set rows and 70 more (two chunks of scanned rows), flipped rows and
    missing values among them; the model and a family K of that N."""
    import skat_ref as R
    from saigegds_amd.gds import pack_dosage_2bit
    mod, sm = M.flat_model(n, kcov, "binary")
    codes = M.hard_calls(n, 77, 11 + n + kcov)
    K, csr, _ = M.family_K(n) if n < 5000 else (None, family_csr(n), None)
    return dict(n=n, sm=sm, codes=codes, packed=pack_dosage_2bit(codes), lut=R.tables(codes), K=K, csr=csr, storage="csr",
                w=np.ascontiguousarray(np.asarray(mod.V, dtype=np.float64)), tau=np.array([1.0, 0.5]), dtype=np.dtype(np.uint8))


def family_csr(n):
    """``skat_kmat_ref.family_K``'s pattern without the dense matrix."""
    rp, col, val = [0], [], []
    for i, sz, empty in M.family_blocks(n):
        for r in range(i, i + sz):
            if not empty:
                col += list(range(i, i + sz))
                val += [1.0 if k == r else 0.5 for k in range(i, i + sz)]
            rp.append(len(col))
    return np.array(rp, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


@pytest.mark.parametrize("kcov", [3, 16])
@pytest.mark.parametrize("n", [1003, 8195])
def test_2_hard_calls_equal_the_2bit_entries_bit_for_bit(n, kcov):
    from saigegds_amd import aggregate
    c = hard_case(n, kcov)
    codes, packed, lut, w, tau = c["codes"], c["packed"], c["lut"], c["w"], c["tau"]
    up, vi = np.array([0, 7, 24, 24, 77], dtype=np.int64), np.arange(77, dtype=np.int32)
    kw = dict(maxiter=KD.MAXITER, tol=1e-9)
    with Dev(c, cap=77) as d:
        want_u = d.sc.skat_kmat(d.op, packed, up, vi, lut, w, tau, **kw)
        want_s = d.sc.cond_kmat_set(d.op, packed[:7], lut[:7], w, tau, **kw)
        want_r = d.sc.cond_kmat(d.op, packed[7:], lut[7:])
        for dtype in (np.uint8, np.float64, np.int32):
            with d.sc.dosage_block(dtype, 77) as blk:
                n_ok, s, _ = blk.load(KD.as_block_rows(codes, dtype))
                flip, mean = aggregate.flip_mean(n_ok, s)
                assert same_bits(aggregate.dosage_tables(flip, mean), lut)
                assert same_units(blk.skat_kmat(d.op, up, vi, flip, mean, w, tau, **kw), want_u), (n, kcov, dtype)
                got_s = blk.cond_kmat_set(d.op, np.arange(7), flip[:7], mean[:7], w, tau, **kw)
                assert same_bits(got_s[0], want_s[0]) and same_bits(got_s[1], want_s[1]) and np.array_equal(got_s[2], want_s[2])
                blk.load(KD.as_block_rows(codes[7:], dtype))
                assert same_rows(blk.cond_kmat(d.op, flip[7:], mean[7:]), want_r), (n, kcov, dtype)
                # the set installed from a block serves sgx_cond_kmat_2bit after the block is reloaded
                assert same_rows(d.sc.cond_kmat(d.op, packed[7:], lut[7:]), want_r)


@pytest.mark.parametrize("name", ["n1003_k16_f64_csr", "n1003_k3_i32_dense", "n61_k1_u8_csr"])
def test_3_a_row_of_the_scan_is_the_last_entry_of_the_unit_set_plus_row(name):
    c = KD.make_case(name)
    C, rows, flip, mean = c["n_cond"], c["rows"], c["flip"], c["mean"]
    m = len(rows)
    with Dev(c) as d:
        d.blk.load(rows)
        S_C, phi_cc, it_c = d.cond_set(np.arange(C), flip[:C], mean[:C])
        S, var, cov, it = d.cond(flip, mean)                       # all loaded rows, the set's own among them
        one = d.skat([0, C], np.arange(C), flip[:C], mean[:C])
        assert same_bits(S_C, one[0]) and same_bits(phi_cc, one[1][0]) and np.array_equal(it_c, one[2])
        js = [j for j in (C, C + 1, m - 2, m - 1) if C <= j < m]
        up = np.arange(len(js) + 1, dtype=np.int64) * (C + 1)
        vi = np.concatenate([list(range(C)) + [j] for j in js]).astype(np.int32)
        su, cu, iu = d.skat(up, vi, flip[vi], mean[vi])
    for k, j in enumerate(js):
        u = cu[k]
        assert same_bits(S[j], su[up[k] + C]) and same_bits(var[j], u[C, C]) and same_bits(cov[j], u[C, :C]), (name, j)
        assert it[j] == iu[up[k] + C]


def test_4_determinism_and_independence():
    c = KD.make_case("n1003_k16_f64_csr")
    C, rows, flip, mean, up, vi = c["n_cond"], c["rows"], c["flip"], c["mean"], c["unit_ptr"], c["var_idx"]
    with Dev(c) as d:
        d.blk.load(rows)
        a, b = d.skat(up, vi, flip, mean), d.skat(up, vi, flip, mean)
        assert same_units(a, b)
        # the unit of 65 alone, behind another unit, and permuted (entry 3 falls into the second 64-column chunk)
        v65 = np.arange(65, dtype=np.int32)
        one = d.skat([0, 65], v65, flip[v65], mean[v65])
        assert same_bits(one[0], a[0][:65]) and same_bits(one[1][0], a[1][0]) and np.array_equal(one[2], a[2][:65])
        v2 = np.concatenate([np.arange(65, 71), v65]).astype(np.int32)
        two = d.skat([0, 6, 71], v2, flip[v2], mean[v2])
        assert same_bits(two[0][6:], one[0]) and same_bits(two[1][1], one[1][0]) and np.array_equal(two[2][6:], one[2])
        perm = np.arange(65)
        perm[[3, 64]] = perm[[64, 3]]
        sp, cp, ip = d.skat([0, 65], v65[perm], flip[perm], mean[perm])
        inv = np.argsort(perm)
        assert same_bits(sp[inv], one[0]) and np.array_equal(ip[inv], one[2]) and same_bits(cp[0][np.ix_(inv, inv)], one[1][0])
        # a row of the scan: its results do not depend on the rows loaded, its position or a set installed before
        d.cond_set(np.arange(C), flip[:C], mean[:C])
        full = d.cond(flip, mean)
        assert same_rows(full, d.cond(flip, mean))
        d.cond_set(np.arange(3), flip[:3], mean[:3])               # another set before
        d.cond_set(np.arange(C), flip[:C], mean[:C])
        pick = np.array([70, 9, 40])
        with d.sc.dosage_block(c["dtype"], 3) as small:
            small.load(rows[pick])
            part = small.cond_kmat(d.op, flip[pick], mean[pick])
        assert same_rows(part, tuple(x[pick] for x in full))


@pytest.mark.parametrize("name", ["n61_k1_u8_csr", "n1003_k3_i32_dense", "n4099_k5_u8_csr"])
def test_5_tau1_zero_is_the_weighted_gram(name):
    from conftest import REL_TOL
    c = KD.make_case(name)
    sm, C, rows, flip, mean = c["sm"], c["n_cond"], c["rows"], c["flip"], c["mean"]
    keep = np.isfinite(mean)
    rows, flip, mean = rows[keep], flip[keep], mean[keep]
    m = len(rows)
    mu2 = np.ones(sm.n) if sm.quant else np.ascontiguousarray(sm.mu2)
    t0 = float(c["tau"][0])
    up, vi = np.array([0, m], dtype=np.int64), np.arange(m, dtype=np.int32)
    with Dev(c) as d:
        d.blk.load(rows)
        score, covs, iters = d.skat(up, vi, flip, mean, tau=[t0, 0.0], w=mu2)
        s2, c2 = d.blk.skat(up, vi, flip, mean)
        _, _, it_c = d.cond_set(np.arange(C), flip[:C], mean[:C], tau=[t0, 0.0], w=mu2)
        S, var, cov, it = d.cond(flip, mean)
        d.blk.cond_set(np.arange(C), flip[:C], mean[:C])
        S2, var2, cov2 = d.blk.cond(flip, mean)
    assert set(np.unique(np.concatenate([iters, it, it_c])).tolist()) <= {0, 1}
    sd = np.sqrt(np.maximum(np.diag(c2[0]), 0))
    f = t0 * sm.var_ratio
    assert np.all(np.abs(f * covs[0] - c2[0]) <= REL_TOL * sd[:, None] * sd[None, :]), name
    assert np.all(np.abs(f * var - var2) <= REL_TOL * sd * sd) and np.all(np.abs(f * cov - cov2) <= REL_TOL * sd[:, None] * sd[None, :C])
    assert np.all(np.abs(S - S2) <= REL_TOL * np.abs(S2) + 1e-9 * np.abs(S2).max())


def test_6_a_non_finite_mean_poisons_its_own_row_and_column():
    c = KD.make_case("n1003_k3_i32_dense")
    rows, flip, mean, up, vi = c["rows"][:-1], c["flip"][:-1], c["mean"][:-1], np.array([0, 17, 40], dtype=np.int64), np.arange(40, dtype=np.int32)
    with Dev(c) as d:
        d.blk.load(rows)
        s0, c0, i0 = d.skat(up, vi, flip[:40], mean[:40])
        for poison in (np.nan, np.inf):
            m2 = mean[:40].copy()
            m2[5] = poison                                         # entry 5 of the unit of 17: no sample of it is missing or all, alike
            s1, c1, i1 = d.skat(up, vi, flip[:40], m2)
            keep = np.arange(40) != 5
            assert np.isnan(s1[5]) and i1[5] == 0 and same_bits(s1[keep], s0[keep]) and np.array_equal(i1[keep], i0[keep])
            k = np.arange(17) != 5
            assert np.all(np.isnan(c1[0][5])) and np.all(np.isnan(c1[0][:, 5])) and same_bits(c1[1], c0[1])
            assert same_bits(c1[0][np.ix_(k, k)], c0[0][np.ix_(k, k)])
        d.cond_set(np.arange(16), flip[:16], mean[:16])
        r0 = d.cond(flip, mean)
        m2 = mean.copy()
        m2[20] = np.nan
        r1 = d.cond(flip, m2)
        keep = np.arange(len(rows)) != 20
        assert np.isnan(r1[0][20]) and np.isnan(r1[1][20]) and np.all(np.isnan(r1[2][20])) and r1[3][20] == 0
        assert same_rows(tuple(x[keep] for x in r1), tuple(x[keep] for x in r0))


def test_7_errors_launch_nothing_and_leave_the_handles_usable():
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner, SgxError
    c = KD.make_case("n61_k1_u8_csr")
    rows, flip, mean, w, tau = c["rows"][:-1], c["flip"][:-1], c["mean"][:-1], c["w"], c["tau"]
    m = len(rows)
    up, vi = np.array([0, 5, m], dtype=np.int64), np.arange(m, dtype=np.int32)
    sm60 = M.flat_model(60, 1, "binary")[1]
    with Dev(c) as d, ExplicitGrmOperator(np.eye(60)) as op60, ExplicitGrmOperator(np.eye(61)) as other, \
            Scanner(sm60) as sc60:
        sc, blk, op, L = d.sc, d.blk, d.op, d.sc._L
        empty = sc.dosage_block(np.uint8, 4)
        blk60 = sc60.dosage_block(np.uint8, 4)
        score, cov, it = np.zeros(m), np.zeros(int((np.diff(up) ** 2).sum())), np.zeros(m, dtype=np.int32)
        var = np.zeros(m)

        def fails(rc, what):
            assert rc == -1 and L.sgx_last_error(), what

        def skat(**kw):
            a = dict(h=sc._h, km=op._h, b=blk._b, up=up.ctypes.data, idx=vi.ctypes.data, flip=flip.ctypes.data,
                     mean=mean.ctypes.data, w=w.ctypes.data, tau=tau.ctypes.data, score=score.ctypes.data, cov=cov.ctypes.data,
                     maxiter=500)
            a.update(kw)
            return L.sgx_ds_block_skat_kmat(a["h"], a["km"], a["b"], len(up) - 1, a["up"], a["idx"], a["flip"], a["mean"], a["w"],
                                            a["tau"], a["maxiter"], 1e-12, a["score"], a["cov"], it.ctypes.data)

        def cset(n_cond=1, **kw):
            a = dict(h=sc._h, km=op._h, b=blk._b, idx=vi.ctypes.data, flip=flip.ctypes.data, mean=mean.ctypes.data,
                     w=w.ctypes.data, tau=tau.ctypes.data, score=score.ctypes.data, cov=cov.ctypes.data, maxiter=500)
            a.update(kw)
            return L.sgx_ds_block_cond_kmat_set(a["h"], a["km"], a["b"], n_cond, a["idx"], a["flip"], a["mean"], a["w"], a["tau"],
                                                a["maxiter"], 1e-12, a["score"], a["cov"], it.ctypes.data)

        def rows_(**kw):
            a = dict(h=sc._h, km=op._h, b=blk._b, flip=flip.ctypes.data, mean=mean.ctypes.data, score=score.ctypes.data,
                     var=var.ctypes.data, cov=cov.ctypes.data)
            a.update(kw)
            return L.sgx_ds_block_cond_kmat(a["h"], a["km"], a["b"], a["flip"], a["mean"], a["score"], a["var"], a["cov"],
                                            it.ctypes.data)

        fails(skat(), "nothing loaded")
        fails(cset(), "nothing loaded")
        blk.load(rows)
        fails(rows_(), "no set")
        good = blk.skat_kmat(op, up, vi, flip, mean, w, tau, tol=KD.TOL_SOLVE)
        for fn, keys in ((skat, ("h", "km", "b", "up", "idx", "flip", "mean", "w", "tau", "score", "cov")),
                         (cset, ("h", "km", "b", "idx", "flip", "mean", "w", "tau", "score", "cov"))):
            for k in keys:
                fails(fn(**{k: None}), k)
            fails(fn(km=op60._h), "another sample count")
            fails(fn(b=blk60._b), "a block of another sample count")
            fails(fn(b=empty._b), "nothing loaded")
            fails(fn(maxiter=-1), "maxiter")
            for bad_w in (0.0, -1.0, np.nan, np.inf):
                w2 = w.copy()
                w2[7] = bad_w
                fails(fn(w=w2.ctypes.data), bad_w)
            for bad_tau in ([0.0, 0.5], [-1.0, 0.5], [1.0, -0.1], [np.nan, 0.1]):
                t2 = np.array(bad_tau)
                fails(fn(tau=t2.ctypes.data), bad_tau)
            for bad_idx in (-1, m):
                v2 = vi.copy()
                v2[0] = bad_idx
                fails(fn(idx=v2.ctypes.data), bad_idx)
        fails(cset(n_cond=17), "n_cond")
        assert np.all(score == 0) and np.all(cov == 0)
        set0 = blk.cond_kmat_set(op, [0, 3], flip[[0, 3]], mean[[0, 3]], w, tau, tol=KD.TOL_SOLVE)
        r0 = blk.cond_kmat(op, flip, mean)
        for k in ("h", "km", "b", "flip", "mean", "score", "var", "cov"):
            fails(rows_(**{k: None}), k)
        fails(rows_(km=other._h), "another matrix than the set's")
        fails(rows_(b=empty._b), "nothing loaded")
        fails(rows_(b=blk60._b), "a block of another sample count")
        with pytest.raises(SgxError, match="no conditioning set"):
            blk60.cond_kmat(op60, np.zeros(0, dtype=np.uint8), np.zeros(0))
        # an installed set stays, both handles stay usable
        assert same_rows(blk.cond_kmat(op, flip, mean), r0)
        assert same_units(blk.skat_kmat(op, up, vi, flip, mean, w, tau, tol=KD.TOL_SOLVE), good)
        again = blk.cond_kmat_set(op, [0, 3], flip[[0, 3]], mean[[0, 3]], w, tau, tol=KD.TOL_SOLVE)
        assert same_bits(again[1], set0[1])
        blk.cond_kmat_set(op, [], [], [], w, tau)                  # n_cond = 0 clears the set
        fails(rows_(), "no set")
        empty.close()
        blk60.close()
