"""sgx_ds_block_collapse on the device (kern_collapse_ds.h) through ``DosageBlock.collapse`` against the
numpy reference of tests/collapse_ds_ref.py, bit for bit, for uint8, int32 and float64 blocks: the rows at every sample
count around a 16-byte piece, a thread's samples and the kernel's slab; group sizes around the unroll; every flip
pattern; special values; counts and table against ``load`` + ``scan`` of the reference's rows in a fresh block; a second
call over earlier pseudo-rows; independence of a group from the other groups; hard calls against ``collapse_2bit``;
``skat`` over a pseudo-row; and the refusals."""
import numpy as np
import pytest

import collapse_ds_ref as DR

pytestmark = pytest.mark.gpu
# kern_collapse_ds.h: a 16-byte piece is 16 uint8 or 2 float64 samples, a thread takes 16 uint8 or 4 float64 samples,
# a workgroup of 256 threads a slab, and a round of the entry loop UNROLL entries
PIECE = {"u8": 16, "f64": 2}
THREAD = {"u8": 16, "f64": 4}
SLAB = {"u8": 256 * 16, "f64": 256 * 4}
UNROLL = {"u8": 8, "f64": 4}
NS = (1, 15, 16, 17, SLAB["f64"] - 1, SLAB["f64"], SLAB["f64"] + 1, SLAB["u8"] - 1, SLAB["u8"], SLAB["u8"] + 1)
SIZES = tuple(sorted({0, 1, 2, 17, 300} | {u + d for u in UNROLL.values() for d in (-1, 0, 1)}))
KINDS = ("u8", "i32", "f64")
DTYPE = {"u8": np.uint8, "i32": np.int32, "f64": np.float64}
M = 40                                                          # rows of a case
_cache = {}


def _model(n):
    from test_gpu_exact import _model as intercept_model
    return intercept_model(n)


def rows_of(n, kind, seed):
    """M rows from the hard calls of ``test_gpu_collapse.rows_of`` (row 0 all missing, row 1 all 0, row 2 all 2, every
    other row alt-major, up to 20 % missing).  f64: two thirds of the values moved to fractions (k / 64), row 3 sprinkled
    with +-Inf, NaN, -0.0, negative values and values above 2.  u8: rows 3 and 4 sprinkled with values 3 .. 254 (row 4 is
    alt-major less often than not: both orientations meet them through the random flips).  i32: row 3 with -1, 3 and 7."""
    from test_gpu_collapse import rows_of as codes_of
    rng = np.random.default_rng(seed)
    codes = codes_of(n, M, seed)
    miss = codes == 3
    if kind == "f64":
        x = codes.astype(np.float64)
        moved = rng.random(x.shape) < 2 / 3
        x = np.where(moved, np.rint(np.clip(x + rng.uniform(-0.4, 0.4, x.shape), 0, 2) * 64) / 64, x)
        x[miss] = np.nan
        x[1], x[2] = 0.0, 2.0
        odd = np.array([np.inf, -np.inf, np.nan, -0.0, -0.5, -2.0, 2.5, 7.0, 5e-324, 1e300])
        at = rng.random(n) < 0.5
        x[3, at] = rng.choice(odd, int(at.sum()))
        return x
    if kind == "u8":
        x = np.where(miss, 0xFF, codes).astype(np.uint8)
        for r in (3, 4):
            at = rng.random(n) < 0.3
            x[r, at] = rng.integers(3, 255, int(at.sum()))
        return x
    x = np.where(miss, DR.NA_INT, codes.astype(np.int64)).astype(np.int32)
    at = rng.random(n) < 0.3
    x[3, at] = rng.choice([-1, 3, 7], int(at.sum()))
    return x


def groups_of(rows, seed, m=M):
    """One group of every size of SIZES with the scan's flips (s > n: mixed), one of every size with random flips, the
    size-17 and size-300 entries again all flipped and all unflipped, the all-missing row alone under both flips, rows 1
    and 2 under both flips and orders, the special rows 3 and 4 alone under both flips, and one group once more -- rows
    are shared by many groups."""
    rng = np.random.default_rng(seed)
    scan_flip = DR.counts_of(rows)[3].astype(np.int64)
    idx = [rng.integers(0, m, k) for k in SIZES]
    flip = [scan_flip[i] for i in idx]
    idx += [rng.integers(0, m, k) for k in SIZES]
    flip += [rng.integers(0, 2, k) for k in SIZES]
    for k in (SIZES.index(17), SIZES.index(300)):
        idx += [idx[k], idx[k]]
        flip += [np.ones(SIZES[k], dtype=np.int64), np.zeros(SIZES[k], dtype=np.int64)]
    idx += [np.array([0]), np.array([0]), np.array([1, 2]), np.array([1, 2]), np.array([2, 1]), idx[2]]
    flip += [np.array([0]), np.array([1]), np.array([0, 0]), np.array([1, 1]), np.array([1, 0]), flip[2]]
    for r in (3, 4):
        idx += [np.array([r]), np.array([r])]
        flip += [np.array([0]), np.array([1])]
    grp_ptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    return grp_ptr, np.concatenate(idx).astype(np.int32), np.concatenate(flip).astype(np.uint8)


def case(n, kind):
    """Per (n, kind), made once and left unchanged: rows, groups, the reference's pseudo-rows."""
    if (n, kind) not in _cache:
        rows = rows_of(n, kind, 100 + n)
        grp_ptr, var_idx, flip = groups_of(rows, 7 + n)
        _cache[n, kind] = (rows, grp_ptr, var_idx, flip, DR.collapse_ds_ref(rows, grp_ptr, var_idx, flip))
    return _cache[n, kind]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def as_input(ref, kind):
    """The reference's pseudo-rows as rows a block of that kind loads (int32: integer-valued, nothing missing)."""
    return ref.astype(np.int32) if kind == "i32" else ref


def test_the_cases_cover_what_they_name():
    assert {s - 1 for s in SLAB.values()} | set(SLAB.values()) | {s + 1 for s in SLAB.values()} <= set(NS)
    assert {1, 15, 16, 17, 4095, 4096, 4097} <= set(NS) and all(n % PIECE["u8"] and n % THREAD["f64"] for n in (15, 17))
    assert {0, 1, 2, 17, 300} <= set(SIZES) and all({u - 1, u, u + 1} <= set(SIZES) for u in UNROLL.values())


@pytest.mark.parametrize("n", NS)
def test_rows_counts_and_table_against_the_reference(n):
    from saigegds_amd._lib import Scanner
    with Scanner(_model(n)) as sc:
        for kind in KINDS:
            rows, grp_ptr, var_idx, flip, ref = case(n, kind)
            ng = len(grp_ptr) - 1
            assert ref.dtype == (np.uint8 if kind == "u8" else np.float64) and set(SIZES) <= set(np.diff(grp_ptr).tolist())
            if n >= 1000:
                assert len({r.tobytes() for r in ref}) > ng // 2      # the groups differ
            with sc.dosage_block(DTYPE[kind], M + 2 * ng) as blk:
                blk.load(rows)
                nv, sm, st, out, valid, got = blk.collapse(grp_ptr, var_idx, flip, return_rows=True)
                assert blk.n_variants == M + ng
                assert same(got, ref), f"N={n} {kind}: rows"
                assert nv.dtype == np.int32 and (nv == n).all()
                # a second call whose groups take earlier pseudo-rows too: they are rows like any other
                rows2 = np.concatenate([DR.resident(rows), ref])
                gp2, vi2, fl2 = groups_of(rows2, 31 + n, m=M + ng)
                ref2 = DR.collapse_ds_ref(rows2, gp2, vi2, fl2)
                assert (vi2 >= M).any()
                got2 = blk.collapse(gp2, vi2, fl2, return_rows=True)
                assert blk.n_variants == M + 2 * ng and same(got2[5], ref2), f"N={n} {kind}: second call"
                assert (got2[0] == n).all()
            with sc.dosage_block(DTYPE[kind], ng) as fresh:         # exactly the reference's rows, loaded and scanned
                want = (*fresh.load(as_input(ref, kind)), *fresh.scan())
            for a, b, nm in zip((nv, sm, st, out, valid), want, ("n_valid", "sum", "sum_trunc", "table", "valid")):
                assert same(a, b), f"N={n} {kind}: {nm}"
            if n >= 1000:
                assert valid.any() and not valid.all()              # (a group of no entries is monomorphic)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_a_group_does_not_depend_on_the_other_groups(kind):
    """Groups alone, in reverse order, repeated and permuted: the same bits per group."""
    from saigegds_amd._lib import Scanner
    n = SLAB["u8"] + 1
    rows, grp_ptr, var_idx, flip, ref = case(n, kind)
    ng = len(grp_ptr) - 1
    ent = [np.arange(grp_ptr[g], grp_ptr[g + 1]) for g in range(ng)]
    orders = [[g] for g in range(ng)] + [list(range(ng))[::-1], [4, 4, 0, 4, 3, 0], list(np.random.default_rng(3).permutation(ng)) * 2]
    with Scanner(_model(n)) as sc, sc.dosage_block(DTYPE[kind], M + sum(len(o) for o in orders)) as blk:
        blk.load(rows)
        for order in orders:
            e = np.concatenate([ent[g] for g in order]) if len(order) else np.zeros(0, dtype=np.int64)
            gp = np.concatenate([[0], np.cumsum([ent[g].size for g in order])]).astype(np.int64)
            got = blk.collapse(gp, var_idx[e], flip[e], return_rows=True)[5]
            assert same(got, ref[order]), order


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_hard_calls_equal_collapse_2bit(kind):
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    from test_gpu_collapse import rows_of as codes_of
    n = 1000
    codes = codes_of(n, M, 5)
    rows = np.where(codes == 3, 0xFF, codes).astype(np.uint8) if kind == "u8" else np.where(codes == 3, np.nan, codes.astype(np.float64))
    grp_ptr, var_idx, flip = groups_of(rows, 9)
    with Scanner(_model(n)) as sc:
        rows2, counts = sc.collapse_2bit(pack_dosage_2bit(codes), grp_ptr, var_idx, flip)
        with sc.dosage_block(DTYPE[kind], M + len(grp_ptr) - 1) as blk:
            blk.load(rows)
            nv, sm, st, _, _, got = blk.collapse(grp_ptr, var_idx, flip, return_rows=True)
    assert np.array_equal(got, unpack_dosage_2bit(rows2, n)) and counts.any()
    assert np.array_equal(sm, counts[:, 0] + 2.0 * counts[:, 1]) and np.array_equal(st, counts[:, 0] + 2 * counts[:, 1])


@pytest.mark.parametrize("kind", KINDS)
def test_skat_on_a_unit_that_ends_in_the_pseudo_row(kind):
    """``blk.skat`` sees the pseudo-row as an ordinary row: a unit of three rows and the pseudo-row of a group equals
    the same unit on a fresh block that stores the reference's row."""
    from saigegds_amd._lib import Scanner
    import skat_ds_ref as D
    n = SLAB["f64"] + 1
    rows, grp_ptr, var_idx, flip, ref = case(n, kind)
    g = int(np.flatnonzero(np.diff(grp_ptr) == 17)[0])
    a, b = int(grp_ptr[g]), int(grp_ptr[g + 1])
    stored = np.concatenate([rows, as_input(ref[g:g + 1], kind)])
    fl, mean = D.flip_mean(stored[[5, 6, 7, M]])
    unit = (np.array([0, 4]), np.array([5, 6, 7, M], dtype=np.int32), fl, mean)
    with Scanner(_model(n)) as sc:
        with sc.dosage_block(DTYPE[kind], M + 1) as blk:
            blk.load(rows)
            blk.collapse([0, b - a], var_idx[a:b], flip[a:b])
            got = blk.skat(*unit)
        with sc.dosage_block(DTYPE[kind], M + 1) as blk:
            blk.load(stored)
            want = blk.skat(*unit)
    assert same(got[0], want[0]) and same(got[1][0], want[1][0]) and np.isfinite(got[0]).all() and got[1][0][3, 3] > 0


def test_refusals_leave_handle_and_block_usable():
    """Every refusal that can be reached from one process on one device (a twin handle and a second device cannot)."""
    from saigegds_amd._lib import Scanner, load
    n, kind = 17, "f64"
    rows, grp_ptr, var_idx, flip, ref = case(n, kind)
    ng, nnz, L = len(grp_ptr) - 1, var_idx.size, load()
    bad_idx = [var_idx.copy() for _ in range(3)]
    bad_idx[0][5], bad_idx[1][nnz - 1], bad_idx[2][0] = M, -1, np.iinfo(np.int32).max
    bad_ptr = [grp_ptr.copy() for _ in range(3)]
    bad_ptr[0][3], bad_ptr[1][0], bad_ptr[2][ng] = grp_ptr[4] + 1, 1, grp_ptr[ng - 1] - 1      # descends, starts at 1, descends at the end
    nv, sm, st = np.full(ng, -1, dtype=np.int32), np.full(ng, -1.0), np.full(ng, -1, dtype=np.int64)
    out, valid, got = np.full((ng, 8), -1.0), np.full(ng, 7, dtype=np.uint8), np.full((ng, n), -1.0)
    with Scanner(_model(n)) as sc, Scanner(_model(n + 1)) as other, sc.dosage_block(np.float64, M + ng) as blk:
        h, b = sc._h, blk._b
        ok = [ng, grp_ptr.ctypes.data, var_idx.ctypes.data, flip.ctypes.data, nv.ctypes.data, sm.ctypes.data, st.ctypes.data,
              out.ctypes.data, valid.ctypes.data, got.ctypes.data]
        assert L.sgx_ds_block_collapse(h, b, *ok) == -1           # nothing loaded
        blk.load(rows)
        cases = [(i, None) for i in range(1, 9)]                  # a NULL buffer (out_rows may be NULL)
        cases += [(2, x.ctypes.data) for x in bad_idx] + [(1, x.ctypes.data) for x in bad_ptr]
        for i, val in cases:
            args = list(ok)
            args[i] = val
            assert L.sgx_ds_block_collapse(h, b, *args) == -1, (i, val)
        assert L.sgx_ds_block_collapse(None, b, *ok) == -1 and L.sgx_ds_block_collapse(h, None, *ok) == -1
        assert L.sgx_ds_block_collapse(other._h, b, *ok) == -1    # a handle of another sample count
        big = np.zeros(ng + 2, dtype=np.int64)                    # one group more than the block has room for
        assert L.sgx_ds_block_collapse(h, b, ng + 1, big.ctypes.data, *ok[2:]) == -1
        assert L.sgx_ds_block_collapse(h, b, 0, *([None] * 9)) == 0                             # no group: nothing to do
        assert blk.n_variants == M and (nv == -1).all() and (out == -1).all() and (valid == 7).all() and (got == -1).all()
        with pytest.raises(ValueError, match="DosageBlock.collapse"):
            blk.collapse(grp_ptr, var_idx, flip[:-1])
        # a good call on the same handle and block
        assert L.sgx_ds_block_collapse(h, b, *ok) == 0
        assert same(got, ref) and (nv == n).all()
        blk.n_variants += ng
        assert blk.scan()[1].shape == (M + ng,)
        assert L.sgx_ds_block_collapse(h, b, 1, big.ctypes.data, *ok[2:]) == -1                 # the block is full now
        blk.load(rows)                                            # the next load resets the block
        assert same(blk.collapse(grp_ptr, var_idx, flip, return_rows=True)[5], ref)
