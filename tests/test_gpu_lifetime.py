"""Ownership of device and pinned memory (csrc/host_mem.h): every object gives back what it took, and a workspace
that regrows between calls leaves the results as they were.

``sgx_live_bytes`` counts the bytes held by every DevBuf / PinBuf of the process.  Each case records it, runs a
sequence of calls on the 1 000-sample golden model (row counts of at most 4 096), and expects the count above the
recorded value while the objects are open and back at it after ``close()``.  No case provokes a failure: that no
failure path skips a release follows from the owners being members and locals (see the header).
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1000


@pytest.fixture(scope="module")
def data(grm1k):
    """The golden rows with what the calls below need per row: dosage table, float64 / uint8 dosages."""
    from saigegds_amd.gds import unpack_dosage_2bit
    packed = np.ascontiguousarray(grm1k["packed"][:4096])
    codes = unpack_dosage_2bit(packed[:512], N)
    f64 = codes.astype(np.float64)
    f64[codes == 3] = np.nan
    u8 = codes.astype(np.uint8)
    u8[codes == 3] = 0xFF
    lut = np.tile(np.array([0.0, 1.0, 2.0, 0.25]), (4096, 1))
    return dict(packed=packed, f64=f64, u8=u8, lut=lut)


def _dev_rows(sc, packed):
    """rows on the device at the scanner's row stride, with buffers for a table -> (rows, bpv, out, valid)"""
    import torch
    dev = torch.device("cuda", 0)
    bpv = sc.row_stride()
    rows = torch.zeros((packed.shape[0], bpv), dtype=torch.uint8, device=dev)
    rows[:, :packed.shape[1]] = torch.from_numpy(packed).to(dev)
    out = torch.zeros((packed.shape[0], 8), dtype=torch.float64, device=dev)
    valid = torch.zeros(packed.shape[0], dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return rows, bpv, out, valid


def _units(m):
    return np.array([0, m], dtype=np.int64), np.arange(m, dtype=np.int32)


def _seq_scanner(model_bin, data, opened):
    from saigegds_amd._lib import Block, Scanner
    pk, lut = data["packed"], data["lut"]
    sc = Scanner(model_bin)
    sc.scan_2bit(pk[:300])
    sc.scan_u8(data["u8"][:64])
    sc.scan_f64(data["f64"][:64])
    sc.burden_2bit(pk[:60], np.array([0, 20, 60], dtype=np.int64), np.arange(60, dtype=np.int32), lut[:60])
    sc.skat_2bit(pk[:40], *_units(40), lut[:40])
    sc.cond_set(pk[:3], lut[:3])
    sc.cond_2bit(pk[100:400], lut[100:400])
    sc.set_option("lanes", 2)
    blk = Block(N, 512)
    sc.load_block(blk, pk[:512])
    rows, bpv, out, valid = _dev_rows(sc, pk[:512])
    sc.scan_block(blk, out.data_ptr(), valid.data_ptr())
    sc.scan_2bit_dev(rows.data_ptr(), bpv, 512, out.data_ptr(), valid.data_ptr())
    sc.sync()
    sc.set_option("lanes", 1)
    opened()
    blk.close()
    sc.close()


def _seq_block(model_bin, data, opened):
    from saigegds_amd._lib import Block, Scanner
    sc = Scanner(model_bin)
    with_scanner = opened.now()
    blk = Block(N, 1024)
    assert opened.now() > with_scanner
    sc.load_block(blk, data["packed"][:1024])
    sc.load_block(blk, data["packed"][1024:1500])
    sc.sync()
    opened()
    held = opened.now()
    blk.close()
    assert opened.now() < held
    sc.close()


def _seq_dosage_block(dtype):
    def run(model_bin, data, opened):
        from saigegds_amd._lib import Scanner
        rows = data["f64"][:200]
        if dtype == np.uint8:
            rows = data["u8"][:200]
        elif dtype == np.int32:
            rows = np.where(np.isnan(rows), np.iinfo(np.int32).min, rows).astype(np.int32)
        m = rows.shape[0]
        flip, mean = np.zeros(m, dtype=np.uint8), np.full(m, 0.25)
        sc = Scanner(model_bin)
        blk = sc.dosage_block(dtype, 256)
        blk.load(rows)
        blk.scan()
        w = np.ones((30, 2))
        blk.burden(np.array([0, 10, 30], dtype=np.int64), np.arange(30, dtype=np.int32), flip[:30], w, w)
        blk.skat(*_units(24), flip[:24], mean[:24])
        blk.cond_set(np.arange(3, dtype=np.int32), flip[:3], mean[:3])
        blk.cond(flip, mean)
        opened()
        blk.close()
        sc.close()
    return run


def _seq_grm(model_bin, data, opened):
    from saigegds_amd._lib import GrmOperator
    rng = np.random.default_rng(5)
    op = GrmOperator(data["packed"][:1536], N)
    w, tau = np.full(N, 0.2), [1.0, 0.5]
    op.pcg_many(w, tau, rng.standard_normal((3, N)), maxiter=20)
    op.set_groups(np.arange(1536) % 4)
    op.pcg_loco(w[None, :], [0, 0], tau, rng.standard_normal((2, N)), [1, -1], maxiter=20)
    op.dense_block(3, 70, 40, 300)
    op.sparse(0.2)
    opened()
    op.close()


def _seq_explicit(kind):
    def run(model_bin, data, opened):
        from saigegds_amd._lib import ExplicitGrmOperator, GrmOperator, Scanner
        rng = np.random.default_rng(6)
        pk, lut = data["packed"], data["lut"]
        with GrmOperator(pk[:1024], N) as g:
            K = g.dense_block(0, N, 0, N)
        K = 0.5 * (K + K.T)
        if kind == "csr":
            keep = (np.abs(K) > 0.1) | np.eye(N, dtype=bool)
            rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
            op = ExplicitGrmOperator(csr=(rp, np.nonzero(keep)[1].astype(np.int32), K[keep]))
        else:
            op = ExplicitGrmOperator(K)
        w, tau = np.full(N, 0.2), [1.0, 0.5]
        op.pcg_many(w, tau, rng.standard_normal((3, N)), maxiter=20)
        sc = Scanner(model_bin)
        sc.skat_kmat(op, pk[:12], np.array([0, 5, 12], dtype=np.int64), np.arange(12, dtype=np.int32), lut[:12], w, tau, maxiter=20)
        opened()
        sc.close()
        op.close()
    return run


def _seq_utilities(model_bin, data, opened):
    from saigegds_amd import _lib
    base = opened.base
    _lib.geno_stats_2bit(data["packed"][:700], N)
    assert _lib.live_bytes() == base
    raw = np.arange(300 * N, dtype=np.int64).reshape(300, N) % 251
    _lib.quantize_packed(raw.astype(np.uint8), "dPackedReal8U", 0.01, 0.0, N, chunk_bytes=64 * N)
    assert _lib.live_bytes() == base
    _lib.check(_lib.load().sgx_selftest(0))
    assert _lib.live_bytes() == base
    opened.skip = True                        # (nothing stays open between these calls)


class _Opened:
    """called where a sequence holds its objects open: the count is above the recorded value"""

    def __init__(self):
        from saigegds_amd import _lib
        self.now = _lib.live_bytes
        self.base = self.now()
        self.seen = self.skip = False

    def __call__(self):
        assert self.now() > self.base
        self.seen = True


@pytest.mark.parametrize("seq", [
    pytest.param(_seq_scanner, id="scanner"),
    pytest.param(_seq_block, id="block"),
    pytest.param(_seq_dosage_block(np.uint8), id="dosage_block_u8"),
    pytest.param(_seq_dosage_block(np.int32), id="dosage_block_i32"),
    pytest.param(_seq_dosage_block(np.float64), id="dosage_block_f64"),
    pytest.param(_seq_grm, id="implicit_grm"),
    pytest.param(_seq_explicit("csr"), id="explicit_grm_csr"),
    pytest.param(_seq_explicit("dense"), id="explicit_grm_dense"),
    pytest.param(_seq_utilities, id="utilities"),
])
def test_live_bytes_return_to_baseline(seq, model_bin, data):
    gc.collect()
    opened = _Opened()
    seq(model_bin, data, opened)
    assert opened.seen or opened.skip
    assert opened.now() == opened.base


def test_close_twice_then_collect(model_bin, data):
    from saigegds_amd._lib import Block, GrmOperator, Scanner, live_bytes
    gc.collect()
    base = live_bytes()
    sc, blk, op = Scanner(model_bin), Block(N, 64), GrmOperator(data["packed"][:512], N)
    dsb = sc.dosage_block(np.float64, 16)
    sc.scan_2bit(data["packed"][:64])
    assert live_bytes() > base
    for o in (dsb, blk, op, sc, dsb, blk, op, sc):
        o.close()
    assert live_bytes() == base
    del sc, blk, op, dsb
    gc.collect()
    assert live_bytes() == base


# ---- a regrown workspace keeps the results ----------------------------------------------------------------------

def _same(a, b):
    """the results of two calls, byte for byte"""
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, (tuple, list)):
            _same(x, y)
        else:
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _regrow(model_bin, call, sizes, prepare=None):
    """call(scanner, size) for each size on ONE scanner equals the same call on a fresh scanner"""
    from saigegds_amd._lib import Scanner
    with Scanner(model_bin) as sc:
        if prepare:
            prepare(sc)
        got = [call(sc, s) for s in sizes]
    for s, g in zip(sizes, got):
        with Scanner(model_bin) as fresh:
            if prepare:
                prepare(fresh)
            _same(g, call(fresh, s))


def test_regrow_scan_2bit(model_bin, data):
    _regrow(model_bin, lambda sc, m: sc.scan_2bit(data["packed"][:m]), [16, 4096, 16])


def test_regrow_scan_f64(model_bin, data):
    _regrow(model_bin, lambda sc, m: sc.scan_f64(data["f64"][:m]), [8, 512, 8])


def test_regrow_skat_2bit(model_bin, data):
    _regrow(model_bin, lambda sc, m: sc.skat_2bit(data["packed"][:m], *_units(m), data["lut"][:m]), [3, 40, 3])


def test_regrow_cond_2bit(model_bin, data):
    """10 rows, then 600: across COND_WG_ROWS = 256"""
    _regrow(model_bin, lambda sc, m: sc.cond_2bit(data["packed"][50:50 + m], data["lut"][50:50 + m]), [10, 600, 10],
            prepare=lambda sc: sc.cond_set(data["packed"][:3], data["lut"][:3]))
