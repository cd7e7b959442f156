"""The case table of test_gpu_score3_shapes.py and its CPU-side model (numpy only: no GPU, no HIP).

score3_kernel (csrc/kern_score3.h) is compiled in 30 shapes: 15 B-fragment counts NBF = 2..16 in the two-plane form
(table S3_FOR_EACH_NBF) and in the three-plane form (S3_FOR_EACH_NBF_MISS).  Which NBF a model gets follows from its
trait, K, N and the range of its columns (limbs_for in host_init.h); s3_plan (s3_layout.h) then cuts the work by tile
group ng, full rounds rf, leftover variant tiles rem and pieces per leftover tile f.  Three functions restate that
library code, so that test_s3_cases.py can show without a GPU that CASES reaches every shape and every plan branch,
and the GPU test can tell a changed rule from a wrong kernel:

  expected_limbs(sm)              limbs_for and the column order of sgx_init
  plan(M, N, grid, form, nbf)     s3_plan with fpw = NAF x NC of the shape tables copied below
  build(case)                     (sm, packed) of a case
"""
from collections import namedtuple

import numpy as np

# ---- the limb rule (mf_fixed.h MF_*, host_init.h limbs_for) -------------------------------------------
MF_NLIMB, MF_LIMB_A, MF_LIMB_E = 7, 5, 6
LD = np.longdouble


def _invert_ld(a):
    """Gauss-Jordan with partial pivoting in long double (fit_xvx_inverse's `invert`) -> inverse, or None."""
    k = a.shape[0]
    a = a.astype(LD).copy()
    inv = np.eye(k, dtype=LD)
    for c in range(k):
        pv = c + int(np.argmax(np.abs(a[c:, c])))
        if not np.abs(a[pv, c]) > 0:
            return None
        a[[c, pv]] = a[[pv, c]]
        inv[[c, pv]] = inv[[pv, c]]
        d = LD(1) / a[c, c]
        a[c] *= d
        inv[c] *= d
        for r in range(k):
            if r != c and a[r, c] != 0:
                f = a[r, c]
                a[r] -= f * a[c]
                inv[r] -= f * inv[c]
    return inv


def derives_c(sm):
    """fit_xvx_inverse (host_init.h): a quantitative model whose t_XVX_inv_XV is t_X times one K x K matrix, to
    1e-13 of its largest entry, does not carry the c' columns (the epilogue forms them from the e columns)."""
    if not sm.quant:
        return False
    x, t = sm.t_X.astype(LD), sm.t_XVX_inv_XV.astype(LD)
    m0 = _invert_ld(np.asarray(sm.XVX))
    if m0 is None:
        return False
    r = t - x @ m0
    gi = _invert_ld(x.T @ x)
    if gi is None:
        return False
    m = m0 + gi @ (x.T @ r)
    worst, scale = np.abs(x @ m - t).max(), np.abs(t).max()
    return bool(worst <= LD(1e-13) * scale) and bool(np.isfinite(m.astype(np.float64)).all())


Limbs = namedtuple("Limbs", "limbs used nbf range_ok")


def expected_limbs(sm):
    """The limb count of every fixed-point column in sgx_score_layout's order (c' (K), e (K), s, w; 0: not carried),
    the columns used (those limbs and the constant column), NBF = ceil(used / 16) + 1 (the value fragments and the
    bit-1 fragment), and whether every column's range max / mean|.| stays within 2^22 (if not, the model takes the
    FP64 kernels and has no shape at all)."""
    n, k = sm.n, sm.k
    assert n * 4.0 * 384.0 < 2147483647.0, "beyond the fixed-point path's sample count"
    w = np.ones(n) if sm.quant else sm.mu2
    cols = np.concatenate([sm.t_XVX_inv_XV, w[:, None] * sm.t_X, sm.y_mu[:, None], w[:, None]], axis=1)   # F of sgx_init
    cs, cw = 2 * k, 2 * k + 1
    order = [cs, cw] + [k + j for j in range(k)] + ([] if derives_c(sm) else list(range(k)))
    limbs = np.zeros(2 * k + 2, dtype=np.int32)
    range_ok = True
    for c in order:
        if c == cw and sm.quant:
            limbs[c] = 1
            continue
        a = np.abs(cols[:, c])
        total = a.astype(LD).sum()
        rng = float(a.max()) / float(total / n) if total > 0 else 1.0
        if not rng <= 4194304.0:
            range_ok = False
        nl = MF_NLIMB if c >= 2 * k else (MF_LIMB_E if c >= k else MF_LIMB_A)
        if rng > 64.0:
            nl = max(nl, MF_LIMB_E)
        if rng > 16384.0:
            nl = MF_NLIMB
        if n < 16384:
            nl = min(MF_NLIMB, nl + 1)
        limbs[c] = nl
    used = 1 + int(limbs.sum())
    return Limbs(limbs, used, (used + 15) // 16 + 1, range_ok)


# ---- the shape tables (kern_score3.h) and the work plan (s3_layout.h) ------------------------------------------
# (NBF, NAF, NC, NLA, NLB, DA, DB): B fragments, A fragments per consumer wave, consumer / row-loader / B-loader
# waves, pairs of row tiles ahead, B tiles ahead.  test_s3_cases.py holds this copy against the header's text.
SHAPES = {
    0: [(2, 4, 8, 3, 1, 1, 2), (3, 4, 8, 3, 1, 1, 1), (4, 4, 8, 3, 1, 1, 1), (5, 3, 8, 3, 1, 1, 2), (6, 3, 8, 3, 1, 1, 1),
        (7, 4, 4, 2, 2, 2, 1), (8, 4, 4, 2, 2, 2, 1), (9, 4, 4, 2, 2, 1, 1), (10, 4, 4, 2, 2, 1, 1), (11, 4, 4, 2, 2, 1, 1),
        (12, 3, 4, 2, 2, 1, 1), (13, 3, 4, 2, 2, 1, 1), (14, 2, 4, 2, 2, 2, 1), (15, 2, 4, 2, 2, 1, 1), (16, 2, 4, 2, 2, 1, 1)],
    1: [(2, 4, 8, 3, 1, 1, 2), (3, 3, 8, 3, 1, 1, 2), (4, 3, 8, 3, 1, 1, 2), (5, 2, 8, 3, 1, 2, 2), (6, 3, 4, 2, 2, 2, 1),
        (7, 2, 4, 2, 2, 2, 1), (8, 2, 4, 2, 2, 2, 1), (9, 2, 4, 2, 2, 2, 1), (10, 2, 4, 2, 2, 2, 1), (11, 1, 4, 2, 2, 2, 1),
        (12, 1, 4, 2, 2, 2, 1), (13, 1, 4, 2, 2, 2, 1), (14, 1, 4, 2, 2, 2, 1), (15, 1, 4, 2, 2, 2, 1), (16, 1, 4, 2, 2, 2, 1)],
}
SHAPE_MACRO = {0: "S3_FOR_EACH_NBF", 1: "S3_FOR_EACH_NBF_MISS"}      # form (the "three_plane" option) -> table


def fpw(form, nbf):
    """16-variant fragments per workgroup = NAF x NC of the form's shape for nbf B fragments."""
    (s,) = [s for s in SHAPES[form] if s[0] == nbf]
    return s[1] * s[2]


def ntile_of(n):
    """256-sample tiles of a row, in whole 128-byte lines (host_init.h, host_blocks.h)."""
    return 2 * ((n + 511) // 512)


def grid_of(n_cu):
    """workgroups of the contraction kernel (host_scan.h)"""
    return max(8, n_cu & ~7)


Plan = namedtuple("Plan", "ntile nfrag fpw vt ng wpg rf rem f ipg")


def plan(M, N, grid, form, nbf):
    """s3_plan for M variants of N samples on `grid` workgroups in the form's shape for nbf B fragments."""
    ntile, w = ntile_of(N), fpw(form, nbf)
    nfrag = (M + 15) // 16
    vt = (nfrag + w - 1) // w
    ng = 8
    while ng > 1 and ntile // ng < 8:
        ng >>= 1
    wpg = grid // ng
    rf, rem = vt // wpg, vt % wpg
    f = 0
    if rem:
        bylen = max(1, (ntile // ng) // 4)
        f = max(1, min(wpg // rem, bylen))
    return Plan(ntile, nfrag, w, vt, ng, wpg, rf, rem, f, rf * wpg + rem * f)


# ---- the cases --------------------------------------------------------------------------------------------------
# m: "tile" = one variant tile of the larger of the two forms' tiles and 17 variants (a full tile and a ragged one
# that the plan cuts into pieces), or (form, a, b, ragged): (a wpg + b) variant tiles of that form and, if ragged, 5
# variants more -- what puts a branch of the plan in reach; M: m at grid = 256, where wpg = 256 / ng.  branch: what
# of `reached` the case is in the table for.  heavy: the model of _heavy_model.
Case = namedtuple("Case", "name trait k n m M miss seed nbf branch heavy", defaults=(False,))

N_S, N_L = 3001, 16_411            # below / from 16 384 samples on: one limb more per column / the reduced widths

CASES = [
    # every NBF in the small class (above 13 it is the only one that reaches it) ...
    Case("q1", "quantitative", 1, N_S, "tile", 529, 0.010, 101, 2, "ng1"),
    Case("b1", "binary", 1, N_S, "tile", 529, 0.010, 102, 3, "ng1"),
    Case("b2", "binary", 2, N_S, "tile", 529, 0.020, 103, 4, "ng1"),
    Case("b3", "binary", 3, N_S, "tile", 401, 0.010, 104, 5, "ng1"),
    Case("b4", "binary", 4, N_S, "tile", 401, 0.003, 105, 6, "ng1"),
    Case("b6", "binary", 6, N_S, "tile", 273, 0.010, 106, 7, "ng1"),
    Case("b7", "binary", 7, N_S, "tile", 273, 0.020, 107, 8, "ng1"),
    Case("b8", "binary", 8, N_S, "tile", 273, 0.010, 108, 9, "ng1"),
    Case("b9", "binary", 9, N_S, "tile", 273, 0.003, 109, 10, "ng1"),
    Case("b10", "binary", 10, N_S, "tile", 273, 0.010, 110, 11, "ng1"),
    Case("b12", "binary", 12, N_S, "tile", 209, 0.020, 111, 12, "ng1"),
    Case("b13", "binary", 13, N_S, "tile", 209, 0.010, 112, 13, "ng1"),
    Case("b14", "binary", 14, N_S, "tile", 145, 0.010, 113, 14, "ng1"),
    Case("b15", "binary", 15, N_S, "tile", 145, 0.020, 114, 15, "ng1"),
    Case("b16-heavy", "binary", 16, N_S, "tile", 145, 0.010, 115, 16, "ng1", True),
    # ... the large class at K other than 3 and 5 ...
    Case("Q1", "quantitative", 1, N_L, "tile", 529, 0.010, 121, 2, "ng8"),
    Case("Q16", "quantitative", 16, N_L, "tile", 273, 0.010, 122, 8, "ng8"),
    Case("B9", "binary", 9, N_L, "tile", 273, 0.010, 123, 9, "ng8"),
    Case("B11", "binary", 11, N_L, "tile", 273, 0.020, 124, 10, "ng8"),
    Case("B16", "binary", 16, N_L, "tile", 209, 0.010, 125, 13, "ng8"),
    # ... and the plan: two and four tile groups, rows too short to cut a leftover tile,
    Case("ng2", "binary", 5, 5000, "tile", 401, 0.010, 131, 6, "ng2"),
    Case("ng4", "quantitative", 6, 9001, "tile", 401, 0.010, 132, 5, "ng4"),
    Case("short-rows", "binary", 2, 700, "tile", 529, 0.010, 133, 4, "f1-short"),
    # a full round and leftover tiles in either form, a full round and no leftover, and more leftover tiles than
    # half the group's workgroups (not cut)
    Case("rounds-three", "binary", 12, N_L, (1, 1, 1, True), 2117, 0.010, 134, 11, "rf-rem-three"),
    Case("rounds-two", "binary", 14, N_L, (0, 1, 1, True), 6341, 0.003, 135, 12, "rf-rem-two"),
    Case("rem0-three", "binary", 12, N_L, (1, 1, 0, False), 2048, 0.010, 136, 11, "rem0-three"),
    Case("uncut-three", "binary", 12, N_L, (1, 0.5, 4, False), 1280, 0.010, 137, 11, "f1-rem-three"),
]
BRANCHES = {"ng1", "ng2", "ng4", "ng8", "rf-rem-two", "rf-rem-three", "rem0-three", "f1-short", "f1-rem-three", "cut"}


def case_id(c):
    return c.name


def variants(c, grid=256):
    """M of the case where the contraction kernel has `grid` workgroups (c.M at 256)."""
    if c.m == "tile":
        return 16 * max(fpw(0, c.nbf), fpw(1, c.nbf)) + 17
    form, a, b, ragged = c.m
    wpg = grid // plan(1, c.n, grid, form, c.nbf).ng
    return (int(a * wpg) + b) * 16 * fpw(form, c.nbf) + (5 if ragged else 0)


def reached(c, grid=256, M=None):
    """The branches of s3_plan that the case takes on `grid` workgroups, as labels (those of a form end in its name)."""
    M = variants(c, grid) if M is None else M
    out = set()
    for form, name in ((0, "two"), (1, "three")):
        p = plan(M, c.n, grid, form, c.nbf)
        out.add(f"ng{p.ng}")
        if p.rf >= 1 and p.rem > 0:
            out.add(f"rf-rem-{name}")
        if p.rf >= 1 and p.rem == 0:
            out.add(f"rem0-{name}")
        if p.f > 1:
            out.add(f"cut-{name}")
        if p.f == 1 and p.ntile // p.ng < 8:
            out.add(f"f1-short-{name}")
        if p.f == 1 and p.ntile // p.ng >= 8 and p.rem > p.wpg // 2:
            out.add(f"f1-rem-{name}")
    for b in ("cut", "f1-short"):            # (in both forms)
        if {f"{b}-two", f"{b}-three"} <= out:
            out.add(b)
    return out


def _heavy_model(n, k, seed):
    """A binary model with three heavy-tailed covariates: two samples each, a case and a control, at 10^4 times the
    column's scale, no effect on the trait.  (A single far sample is a leverage point: the fit reproduces its y,
    its weight mu (1 - mu) all but vanishes and takes the column's range with it; a case and a control at the same
    value keep their fitted mean at 1/2.)  The fit runs in scaled columns, the model keeps the raw ones.  Each such
    covariate widens its c' column to seven limbs, which is what takes K = 16 from 15 B fragments to 16."""
    from saigegds_amd.nullmod import NullModel, init_nullmod
    rng = np.random.default_rng(seed)
    X = np.ones((n, k))
    for j in range(1, k):
        X[:, j] = rng.standard_normal(n) if j % 2 == 1 else rng.integers(0, 2, n)
    heavy = (1, 3, 5)
    bcov = np.full(k - 1, 0.5)
    bcov[[j - 1 for j in heavy]] = 0.0
    lin = X[:, 1:] @ bcov
    lo, hi = -20.0, 20.0
    for _ in range(80):                        # the intercept of a prevalence of 0.1
        b0 = 0.5 * (lo + hi)
        lo, hi = (lo, b0) if np.mean(1 / (1 + np.exp(-(b0 + lin)))) > 0.1 else (b0, hi)
    y = (rng.random(n) < 1 / (1 + np.exp(-(b0 + lin)))).astype(np.float64)
    cases, controls = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
    for a, j in enumerate(heavy):
        X[[cases[7 + a], controls[7 + a]], j] = 1e4
    sc = np.abs(X).max(0)
    Xs = X / sc
    beta = np.zeros(k)
    for _ in range(100):
        mu = 1 / (1 + np.exp(-(Xs @ beta)))
        step = np.linalg.solve(Xs.T @ (Xs * (mu * (1 - mu))[:, None]), Xs.T @ (y - mu))
        beta += step
        if np.max(np.abs(step)) < 1e-12:
            break
    mu = 1 / (1 + np.exp(-(Xs @ beta)))
    V = mu * (1 - mu)
    vr = 0.94105067
    mod = NullModel(trait_type="binary", tau=np.array([1.0, 0.0]), fitted_values=mu, sample_id=[f"s{i + 1}" for i in range(n)],
                    var_ratio=np.array([vr]), y=y, V=V, X1=X, XV=(X * V[:, None]).T,
                    XXVX_inv=X @ np.linalg.inv(X.T @ (X * V[:, None])), coefficients=beta / sc)
    return init_nullmod(mod, np.arange(n), float("nan"), 10, 0.1, 0.05, vr)


def build_model(c):
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    if c.heavy:
        return _heavy_model(c.n, c.k, c.seed)
    mod = synth.synth_null_model(c.n, c.trait, 0.1 if c.trait == "binary" else 0.0, n_cov=c.k, seed=c.seed)
    return init_nullmod(mod, np.arange(c.n), float("nan"), 10, 0.1, 0.05, float(mod.var_ratio[0]))


def build_rows(c, m=None):
    """m rows (default: the case's own count) with 30 % of the variants flipped and the case's missing rate: the
    three-plane form's third plane and the two-plane form's lists both carry data."""
    from saigegds_amd import synth
    m = c.M if m is None else m
    thr = synth.variant_thresholds(0, m, c.seed, log10_maf=(-2.5, -0.3), flip_frac=0.3, miss_rate=c.miss)
    return synth.synth_packed(c.n, 0, m, c.seed, thr)


def build(c, m=None):
    """(sm, packed) of a case, as test_gpu_parity._synthetic_case makes them"""
    return build_model(c), build_rows(c, m)
