"""sgx_collapse_2bit(_dev) on the device (kern_collapse.h) against the numpy reference of
tests/collapse_ref.py, bit for bit: rows and counts at every sample count around a word, a 16-byte piece and the
kernel's slab of 16 384 samples, group sizes 0 / 1 / 2 / 17 / 300, every flip pattern, garbage in the padding, longer
rows, several upload chunks, the device entry, independence of a group from the other groups, and the errors."""
import numpy as np
import pytest

import collapse_ref as CR

pytestmark = pytest.mark.gpu
SLAB = 16384                                                    # samples of COLLAPSE_SLAB bytes (kern_collapse.h)
NS = (1, 3, 4, 5, 63, 64, 65, 255, 257, 1000, SLAB - 1, SLAB, SLAB + 1)
SIZES = (0, 1, 2, 17, 300)
M = 40                                                          # rows of a case
_cache = {}


def _model(n):
    from test_gpu_exact import _model as intercept_model
    return intercept_model(n)


def rows_of(n, m, seed):
    """m rows of codes: minor allele frequencies 0.0005 to 0.3 (so that the maximum over 300 rows still holds 0s, 1s and
    2s), every other row alt-major, 0 to 20 % missing; row 0 is all missing, row 1 all 0, row 2 all 2."""
    rng = np.random.default_rng(seed)
    f = rng.choice([0.0005, 0.002, 0.01, 0.3], m, p=[0.4, 0.3, 0.2, 0.1])[:, None]
    u = rng.random((m, n))
    codes = ((u < f * f).astype(np.uint8) + (u < 1 - (1 - f) ** 2)).astype(np.uint8)
    codes[1::2] = 2 - codes[1::2]
    codes[rng.random((m, n)) < rng.choice([0, 0.01, 0.2], m)[:, None]] = 3
    codes[0], codes[1], codes[2] = 3, 0, 2
    return codes


def garbage_beyond(packed, n):
    """The fields beyond sample n - 1 in the row's last byte set (to missing codes)."""
    packed = packed.copy()
    if n % 4:
        packed[:, (n + 3) // 4 - 1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)
    return packed


def case(n):
    """Per n, made once: packed rows (tight, garbage beyond sample n - 1), the groups and the reference's result.
    Groups: one of every size of SIZES with the scan's flips (s > n: a mixed-flip group), one of every size with random
    flips, then the size-17 and size-300 entries again all flipped and all unflipped, the all-missing row alone (flipped
    and not), rows 1 and 2 under both flips, and the first group of two once more -- rows are shared by many groups."""
    if n not in _cache:
        from saigegds_amd.gds import pack_dosage_2bit
        rng = np.random.default_rng(7 + n)
        codes = rows_of(n, M, 100 + n)
        packed = garbage_beyond(pack_dosage_2bit(codes), n)
        idx = [rng.integers(0, M, k) for k in SIZES]
        flip = [CR.counts_of(codes)[3][i].astype(np.int64) for i in idx]
        idx += [rng.integers(0, M, k) for k in SIZES]
        flip += [rng.integers(0, 2, k) for k in SIZES]
        for k in (3, 4):
            idx += [idx[k], idx[k]]
            flip += [np.ones(SIZES[k], dtype=np.int64), np.zeros(SIZES[k], dtype=np.int64)]
        idx += [np.array([0]), np.array([0]), np.array([1, 2]), np.array([1, 2]), np.array([2, 1]), idx[2]]
        flip += [np.array([0]), np.array([1]), np.array([0, 0]), np.array([1, 1]), np.array([1, 0]), flip[2]]
        grp_ptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
        var_idx, flip = np.concatenate(idx).astype(np.int32), np.concatenate(flip).astype(np.uint8)
        _cache[n] = (packed, grp_ptr, var_idx, flip, *CR.collapse_ref(packed, n, grp_ptr, var_idx, flip))
    return _cache[n]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev_call(sc, packed, grp_ptr, var_idx, flip, extra=0, fill=0):
    """The rows through sgx_collapse_2bit_dev at the device stride (+ extra bytes), the bytes beyond the host row `fill`
    -> (rows [n_groups, stride], counts); the result buffers start out as 0xAA bytes and -1."""
    import torch
    m, stride, ng = packed.shape[0], sc.row_stride() + extra, len(grp_ptr) - 1
    rows = torch.full((m, stride), fill, dtype=torch.uint8)
    rows[:, :packed.shape[1]] = torch.from_numpy(np.ascontiguousarray(packed))
    rows = rows.cuda()
    gp, vi = torch.from_numpy(np.ascontiguousarray(grp_ptr)).cuda(), torch.from_numpy(np.ascontiguousarray(var_idx)).cuda()
    fl = torch.from_numpy(np.ascontiguousarray(flip)).cuda()
    out = torch.full((ng, stride), 0xAA, dtype=torch.uint8, device="cuda")
    cnt = torch.full((ng, 2), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sc.collapse_2bit_dev(rows.data_ptr(), stride, m, ng, gp.data_ptr(), vi.data_ptr(), fl.data_ptr(), out.data_ptr(), cnt.data_ptr())
    sc.sync()
    return out.cpu().numpy(), cnt.cpu().numpy()


def check(got, ref, nb, what):
    """Rows equal to the reference's over the nb = ceil(n / 4) bytes and zero beyond, counts equal."""
    rows, counts = got
    assert rows.dtype == np.uint8 and counts.dtype == np.int32, what
    assert np.array_equal(rows[:, :nb], ref[0][:, :nb]), what
    assert not rows[:, nb:].any(), f"{what}: padding bytes not zero"
    assert np.array_equal(counts, ref[1]), what


@pytest.mark.parametrize("n", NS)
def test_rows_and_counts_against_the_reference(n):
    from saigegds_amd._lib import Scanner
    packed, grp_ptr, var_idx, flip, ref_rows, ref_counts = case(n)
    nb = (n + 3) // 4
    assert packed.shape == (M, nb) and ref_rows.shape == (len(grp_ptr) - 1, nb)
    sizes = np.diff(grp_ptr)
    assert set(SIZES) <= set(sizes.tolist()) and ref_counts[sizes > 2].any()
    if n % 4:
        assert not (ref_rows[:, -1] >> (2 * (n % 4))).any()     # the reference's own padding fields
    with Scanner(_model(n)) as sc:
        got = sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
        assert got[0].shape == ref_rows.shape
        check(got, (ref_rows, ref_counts), nb, f"N={n} host stride ceil(N/4)")
        for fill in (0x55, 0xFF):                               # hets / missing codes in the bytes beyond the row
            wide = np.concatenate([packed, np.full((M, 21), fill, dtype=np.uint8)], axis=1)
            got = sc.collapse_2bit(wide, grp_ptr, var_idx, flip)
            assert got[0].shape == (len(grp_ptr) - 1, nb + 21)
            check(got, (ref_rows, ref_counts), nb, f"N={n} host stride + 21, padding {fill:#x}")
            check(dev_call(sc, packed, grp_ptr, var_idx, flip, extra=64, fill=fill), (ref_rows, ref_counts), nb,
                  f"N={n} device stride + 64, padding {fill:#x}")
        dev = dev_call(sc, packed, grp_ptr, var_idx, flip)
        check(dev, (ref_rows, ref_counts), nb, f"N={n} device stride")
        host = sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
        assert same(dev[0][:, :nb], host[0]) and same(dev[1], host[1])      # the device entry is the host entry


def test_a_group_does_not_depend_on_the_other_groups():
    """Groups alone, in reverse order, repeated, and among groups of other rows: the same bits per group."""
    from saigegds_amd._lib import Scanner
    n = SLAB + 1
    packed, grp_ptr, var_idx, flip, ref_rows, ref_counts = case(n)
    ng = len(grp_ptr) - 1
    ent = [np.arange(grp_ptr[g], grp_ptr[g + 1]) for g in range(ng)]

    def call(sc, order):
        e = np.concatenate([ent[g] for g in order]) if len(order) else np.zeros(0, dtype=np.int64)
        gp = np.concatenate([[0], np.cumsum([ent[g].size for g in order])]).astype(np.int64)
        return sc.collapse_2bit(packed, gp, var_idx[e], flip[e])
    with Scanner(_model(n)) as sc:
        full = call(sc, list(range(ng)))
        assert same(full[0], ref_rows) and same(full[1], ref_counts)
        for g in range(ng):                                     # alone
            one = call(sc, [g])
            assert same(one[0][0], full[0][g]) and same(one[1][0], full[1][g]), g
        for order in (list(range(ng))[::-1], [4, 4, 0, 4, 3, 0], list(np.random.default_rng(3).permutation(ng)) * 2):
            got = call(sc, order)
            assert same(got[0], full[0][order]) and same(got[1], full[1][order]), order
        assert same(call(sc, list(range(ng)))[1], full[1])      # a second call: the counts start from zero again


def test_a_call_in_several_upload_chunks():
    """sgx_collapse_2bit sends its rows up in chunks of pipe_mb MiB at the device stride (256 bytes at N = 1000), so
    pipe_mb = 1 is 4096 rows a chunk: 9000 rows are two chunks and a tail, and groups take rows from all three."""
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 1000, 9000
    rng = np.random.default_rng(21)
    packed = pack_dosage_2bit(rows_of(n, m, 5))
    sizes = rng.choice([0, 1, 2, 17, 300], 60)
    grp_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    var_idx, flip = rng.integers(0, m, grp_ptr[-1]).astype(np.int32), rng.integers(0, 2, grp_ptr[-1]).astype(np.uint8)
    var_idx[:3] = [0, 4096, m - 1]
    ref = CR.collapse_ref(packed, n, grp_ptr, var_idx, flip)
    with Scanner(_model(n)) as sc:
        assert (1 << 20) // sc.row_stride() == 4096 and m > 2 * 4096
        try:
            sc.set_option("pipe_mb", 0)
            one = sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
            sc.set_option("pipe_mb", 1)
            cut = sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
        finally:
            sc.set_option("pipe_mb", 0)
        assert same(one[0], ref[0]) and same(one[1], ref[1]) and same(cut[0], one[0]) and same(cut[1], one[1])
        out, valid = sc.scan_2bit(one[0])                       # a pseudo-row is a source of the scan like any row
        mac = one[1][:, 0] + 2 * one[1][:, 1]
        ok = valid != 0
        assert valid.shape == (60,) and ok.any() and not ok[mac == 0].any()
        assert np.array_equal(np.rint(out[ok, 0] * 2 * out[ok, 2]), mac[ok]) and np.all(out[ok, 2] == n)


def test_refusals_leave_the_handle_usable():
    import torch
    from saigegds_amd._lib import Scanner, load
    n = 257
    packed, grp_ptr, var_idx, flip, ref_rows, ref_counts = case(n)
    ng, nnz, bpv, L = len(grp_ptr) - 1, var_idx.size, packed.shape[1], load()
    bad_idx = [var_idx.copy() for _ in range(3)]
    bad_idx[0][5], bad_idx[1][nnz - 1], bad_idx[2][0] = M, -1, np.iinfo(np.int32).max
    bad_ptr = [grp_ptr.copy() for _ in range(3)]
    bad_ptr[0][3], bad_ptr[1][0], bad_ptr[2][ng] = grp_ptr[4] + 1, 1, grp_ptr[ng - 1] - 1      # descends, starts at 1, descends at the end
    with Scanner(_model(n)) as sc:
        h = sc._h
        rows, counts = np.full((ng, bpv), 0xAA, dtype=np.uint8), np.full((ng, 2), -1, dtype=np.int32)
        ok = [packed.ctypes.data, bpv, M, ng, grp_ptr.ctypes.data, var_idx.ctypes.data, flip.ctypes.data, rows.ctypes.data,
              counts.ctypes.data]
        cases = [(i, None) for i in (0, 4, 5, 6, 7, 8)] + [(1, bpv - 1), (2, 5)]       # NULL; short rows; fewer rows than the indices name
        cases += [(5, b.ctypes.data) for b in bad_idx] + [(4, b.ctypes.data) for b in bad_ptr]
        for i, val in cases:
            args = list(ok)
            args[i] = val
            assert L.sgx_collapse_2bit(h, *args) == -1, (i, val)
        assert L.sgx_collapse_2bit(None, *ok) == -1
        assert L.sgx_collapse_2bit(h, None, bpv, 0, 0, None, None, None, None, None) == 0       # no group: nothing to do
        assert (rows == 0xAA).all() and (counts == -1).all()
        with pytest.raises(ValueError, match="collapse_2bit"):
            sc.collapse_2bit(packed, grp_ptr, var_idx, flip[:-1])
        # the device entry: NULL, stride, alignment, the groups
        stride = sc.row_stride()
        d_rows = torch.zeros((M, stride), dtype=torch.uint8)
        d_rows[:, :bpv] = torch.from_numpy(packed)
        d_rows = d_rows.cuda()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                  # noqa: E731
        gp, vi, fl = up(grp_ptr), up(var_idx), up(flip)
        d_out = torch.full((ng, stride), 0xAA, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((ng, 2), -1, dtype=torch.int32, device="cuda")
        keep = [up(b) for b in bad_idx + bad_ptr]
        torch.cuda.synchronize()
        ok = [d_rows.data_ptr(), stride, M, ng, gp.data_ptr(), vi.data_ptr(), fl.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr()]
        cases = [(i, None) for i in (0, 4, 5, 6, 7, 8)] + [(1, stride - 64), (1, stride + 16), (2, 5)]
        cases += [(0, ok[0] + 4), (7, ok[7] + 4), (4, ok[4] + 4), (5, ok[5] + 2), (8, ok[8] + 2)]
        cases += [(5, t.data_ptr()) for t in keep[:3]] + [(4, t.data_ptr()) for t in keep[3:]]
        for i, val in cases:
            args = list(ok)
            args[i] = val
            assert L.sgx_collapse_2bit_dev(h, *args) == -1, (i, val)
        assert L.sgx_collapse_2bit_dev(None, *ok) == -1
        assert L.sgx_collapse_2bit_dev(h, None, stride, 0, 0, None, None, None, None, None) == 0
        sc.sync()
        assert (d_out.cpu().numpy() == 0xAA).all() and (d_cnt.cpu().numpy() == -1).all()   # nothing was launched
        # good calls on the same handle
        assert L.sgx_collapse_2bit_dev(h, *ok) == 0
        sc.sync()
        check((d_out.cpu().numpy(), d_cnt.cpu().numpy()), (ref_rows, ref_counts), bpv, "the device entry after the refusals")
        assert L.sgx_collapse_2bit(h, packed.ctypes.data, bpv, M, ng, grp_ptr.ctypes.data, var_idx.ctypes.data, flip.ctypes.data,
                                   rows.ctypes.data, counts.ctypes.data) == 0
        assert same(rows, ref_rows) and same(counts, ref_counts)
        out, valid = sc.scan_2bit(packed)                       # the handle still scans
        assert valid.shape == (M,)


def test_memory_returns():
    from saigegds_amd._lib import Scanner, live_bytes
    start = live_bytes()
    packed, grp_ptr, var_idx, flip, ref_rows, _ = case(1000)
    sc = Scanner(_model(1000))
    sc.collapse_2bit(packed, grp_ptr, var_idx, flip)
    held = live_bytes()
    assert held > start
    assert same(sc.collapse_2bit(packed, grp_ptr, var_idx, flip)[0], ref_rows)
    assert live_bytes() == held                                 # no scratch: nothing but the staging buffer of the first call
    sc.close()
    assert live_bytes() == start
