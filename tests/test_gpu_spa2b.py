"""The saddlepoint stage on packed 2-bit rows in the forms the small cases never reach (spa2b_cases.py): rows with more
than SPA5_NNZ = 8192 carriers, which go through the cumulant pass -- spa4_moments<K, 12> / <K, 16> over segments of
spa_seg(K) samples (the LDS-DMA staging of the table and its tail, the wave queues of spa4_qcap(K) entries, both
widths of wave_reduce_scatter) and spa4_solve -- at every covariate count K = 1 .. 16, beside rows of at most 8192
carriers that go to spa5_kernel in the same call; and the forms of spa5_kernel by the length of the packed row that
no other test runs (512 threads with the row staged in LDS below 48 KiB, and the row not staged).  Dosage rows
always start in tier A (test_gpu_ds_spa.py); 2-bit rows are routed by their carrier count.

Full rows against the CPU oracle by the project's 1e-10 rule (conftest.assert_table_close); one path against another
at rtol = 1e-11 on beta / SE / pval / p.norm.  n_spa is compared with the oracle's count of flagged variants, and
spa2b_cases / test_spa2b_cases.py show by the carrier counts which of them the cumulant pass gets.  sgx_stats does
not tell tier A from tier B, and which of the two a variant starts in depends on SPA4_TIER_X applied to the
score-stage sums: that split is NOT asserted here.  The spread of the planted z-scores (2.1 .. 6) is there to
populate both, and the tests assert that the series (either tier, or the per-variant series) answers part of what is
compared instead of handing everything to the exact sweeps."""
import numpy as np
import pytest

import spa2b_cases as S
from conftest import assert_table_close

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

RTOL_PATHS = 1e-11


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _scanner(sm):
    from saigegds_amd._lib import Scanner
    return Scanner(sm, device=0)


def _case(n, m, k):
    sm, packed = S.case(n, m, k)
    ref, ref_valid, flagged = S.reference(n, m, k)
    return sm, packed, ref, ref_valid, int(flagged.sum())


def _check(out, valid, ref, ref_valid, what):
    assert_table_close(out, valid, ref, ref_valid, what=what)
    assert np.isnan(out[ref_valid == 0]).all(), f"{what}: a rejected variant's row is not NaN"


def _same(a, b, ref_valid, what):
    v = ref_valid.astype(bool)
    assert np.array_equal(a[v][:, :3], b[v][:, :3]), f"{what}: AF / mac / num differ"
    np.testing.assert_allclose(a[v][:, 3:7], b[v][:, 3:7], rtol=RTOL_PATHS, err_msg=what)
    assert np.array_equal(a[v][:, 7], b[v][:, 7]), f"{what}: converged differs"


def _scan_block(sc, blk, m):
    """scan of a loaded block into fresh device buffers -> (out, valid) as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    out = torch.full((m, 8), -1.0, dtype=torch.float64, device=dev)
    valid = torch.zeros(m, dtype=torch.uint8, device=dev)
    sc.scan_block(blk, out.data_ptr(), valid.data_ptr())
    sc.sync()
    return out.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("n,m,k", S.SERIES_CASES)
def test_series_tiers_against_the_oracle(n, m, k):
    sm, packed, ref, ref_valid, nflag = _case(n, m, k)
    with _scanner(sm) as sc:
        out, valid = sc.scan_2bit(packed)
        st = sc.stats()
    what = f"N={n} M={m} K={k}"
    print(f"{what}: n_spa {st['n_spa']} (oracle {nflag}), exact sweeps {st['n_spa_slow']}, dense {st['n_spa_dense']}")
    _check(out, valid, ref, ref_valid, what)
    assert st["n_spa"] == nflag, (what, st, nflag)
    # (strong signals go on to the exact sweeps; what the series itself answers has to be part of the comparison)
    assert st["n_spa"] - st["n_spa_slow"] - st["n_spa_dense"] >= 8, (what, st)


@pytest.mark.parametrize("k", S.K_PER_SEG)
def test_series_tiers_from_a_resident_block(k):
    """The same rows resident in a Block: the cumulant pass reads block rows, and spa5_kernel walks the block's carrier
    lists of up to 8192 entries (those over SPA5_BIG = 2048 in its first round) -- or scans the rows where the lists
    are ignored ("spa_scan_rows") or too small for the later variants (clist_avg)."""
    from saigegds_amd._lib import Block
    n, m = S.N_SERIES, 96
    sm, packed, ref, ref_valid, nflag = _case(n, m, k)
    c, _ = S.codes(n, m, k)
    g = S.flagged_groups(n, m, k)
    few = g["flagged"] & ~g["many"]
    nnz = np.array([S.carriers(c[j], g["flip"][j]) for j in np.flatnonzero(few)])
    assert (nnz > 2048).any() and (nnz <= 2048).any(), nnz          # both rounds of spa5_kernel
    what = f"N={n} M={m} K={k} block"
    with _scanner(sm) as sc, Block(sm.n, m) as blk:
        direct, dvalid = sc.scan_2bit(packed)
        _check(direct, dvalid, ref, ref_valid, what + ", row-major call")
        sc.load_block(blk, packed)
        assert blk.n_variants == m
        base, valid = _scan_block(sc, blk, m)
        st = sc.stats()
        _check(base, valid, ref, ref_valid, what)
        assert st["n_spa"] == nflag, (what, st, nflag)
        _same(base, direct, ref_valid, what + " against the row-major call")
        sc.set_option("spa_scan_rows", 1)
        out, valid = _scan_block(sc, blk, m)
        sc.set_option("spa_scan_rows", 0)
        _check(out, valid, ref, ref_valid, what + ", lists ignored")
        _same(out, direct, ref_valid, what + ", lists ignored, against the row-major call")
        # 300 entries per variant: 28 800 in all, and the rare rows have 300 .. 6 700 carriers each
        with Block(sm.n, m, clist_avg=300) as small:
            sc.load_block(small, packed)
            out, valid = _scan_block(sc, small, m)
            st = sc.stats()
        _check(out, valid, ref, ref_valid, what + ", short lists")
        assert st["n_spa"] == nflag, (what, st, nflag)
        _same(out, direct, ref_valid, what + ", short lists, against the row-major call")


@pytest.mark.parametrize("option", ["score_v1", "spa_exact", "force_dense"])
@pytest.mark.parametrize("k", (4, 8, 16))
def test_other_routes(k, option):
    """"score_v1": every flagged variant, the rare ones and FIRST_SEG_ROW (segments without a carrier) included, through
    spa4_moments<K, 12>; "spa_exact": through the exact exp / log sweeps; "force_dense": through the dense pass."""
    n, m = S.N_SERIES, 96
    sm, packed, ref, ref_valid, nflag = _case(n, m, k)
    with _scanner(sm) as sc:
        base, _ = sc.scan_2bit(packed)
        sc.set_option(option, 1)
        out, valid = sc.scan_2bit(packed)
        st = sc.stats()
    what = f"N={n} M={m} K={k} {option}"
    print(f"{what}: n_spa {st['n_spa']} (oracle {nflag}), exact sweeps {st['n_spa_slow']}, dense {st['n_spa_dense']}")
    _check(out, valid, ref, ref_valid, what)
    assert st["n_spa"] == nflag, (what, st, nflag)
    if option == "spa_exact":
        assert st["n_spa_slow"] + st["n_spa_dense"] == nflag, (what, st)
    _same(out, base, ref_valid, what + " against the unforced table")


@pytest.mark.parametrize("n,m,k", S.ROWLEN_CASES)
def test_per_variant_kernel_row_forms(n, m, k):
    sm, packed, ref, ref_valid, nflag = _case(n, m, k)
    with _scanner(sm) as sc:
        out, valid = sc.scan_2bit(packed)
        st = sc.stats()
        sc.set_option("spa_exact", 1)
        exact, evalid = sc.scan_2bit(packed)
        ste = sc.stats()
    what = f"N={n} M={m} K={k}"
    print(f"{what}: n_spa {st['n_spa']} (oracle {nflag}), exact sweeps {st['n_spa_slow']}, dense {st['n_spa_dense']}")
    _check(out, valid, ref, ref_valid, what)
    assert st["n_spa"] == nflag, (what, st, nflag)
    _check(exact, evalid, ref, ref_valid, what + " spa_exact")
    assert ste["n_spa"] == nflag and ste["n_spa_slow"] + ste["n_spa_dense"] == nflag, (what, ste, nflag)
    _same(exact, out, ref_valid, what + " spa_exact against the first table")


@pytest.mark.parametrize("k", S.K_PER_SEG)
def test_two_lanes_same_table(k):
    """Two halves of a case on two lanes: each lane's moments kernel has an item queue of its own (cur5 + 2), put
    back to zero by the last workgroup to leave -- the second call of a lane finds it so, or counts from where the
    first one stopped."""
    import torch
    n, m = S.N_SERIES, 96
    sm, packed, ref, ref_valid, nflag = _case(n, m, k)
    dev = torch.device("cuda", 0)
    with _scanner(sm) as sc:
        one, _ = sc.scan_2bit(packed)
        sc.stats_total(reset=True)
        bpv = sc.row_stride()
        pk = torch.zeros((m, bpv), dtype=torch.uint8, device=dev)
        pk[:, :packed.shape[1]] = torch.from_numpy(packed).to(dev)
        out = torch.full((m, 8), -1.0, dtype=torch.float64, device=dev)
        valid = torch.zeros((m,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sc.set_option("lanes", 2)
        for rep in range(2):                    # every lane twice
            for lo in (0, m // 2):
                sc.scan_2bit_dev(pk[lo:lo + m // 2].data_ptr(), bpv, m // 2, out[lo:lo + m // 2].data_ptr(), valid[lo:lo + m // 2].data_ptr())
            sc.sync()
            tot, _ = sc.stats_total(reset=True)
            assert tot["n_spa"] == nflag, (k, rep, tot, nflag)
        sc.set_option("lanes", 1)
        got, gv = out.cpu().numpy(), valid.cpu().numpy()
    what = f"N={n} M={m} K={k} two lanes"
    _check(got, gv, ref, ref_valid, what)
    _same(got, one, ref_valid, what + " against one lane")
