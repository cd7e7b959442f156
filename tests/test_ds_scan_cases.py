"""CPU: the case table of test_gpu_ds_score.py / test_gpu_ds_spa.py (ds_scan_cases.py) holds what it names -- enough
valid, flipped and rejected variants, the planted rows where the table says, flagged variants in the binary cases and
none at spa_pval = 0 -- and its copies of the library's formulas (tile, split, segment) are the ones in the headers."""
import os

import numpy as np
import pytest

import ds_scan_cases as D
from conftest import ROOT

BIG = [s for s in D.SHAPES if s[1] >= 33]


def _src(name):
    return open(os.path.join(ROOT, "saigegds_amd", "csrc", name)).read()


def test_formulas_are_the_headers():
    """A retuned tile, split or segment rule fails here instead of moving the edges away from the cases unnoticed."""
    assert [D.tile(k) for k in range(1, 9)] == [1024, 640, 512, 384, 320, 256, 256, 192]
    assert "constexpr int TS = ((4096 / P) & ~63) < 64 ? 64 : ((4096 / P) & ~63);" in _src("kern_score.h")
    assert "#define DS_TILE_VB 32 " in _src("kern_score.h")
    host = _src("host_spa.h")
    assert "int ns = std::max(1, std::min((4 * h->n_cu + vb - 1) / vb, (md.N + 4095) / 4096));" in host
    assert "int per = (((md.N + ns - 1) / ns) + 63) & ~63;" in host and "ns = (md.N + per - 1) / per;" in host
    assert "if constexpr (KK <= 8) {" in host
    assert [D.spa_seg(k) for k in (1, 3, 4, 7, 8, 15, 16)] == [4096, 4096, 2048, 2048, 1024, 1024, 512]
    assert "const int full = row <= 32 ? 4096 : row <= 64 ? 2048 : row <= 128 ? 1024 : 512;" in _src("kern_spa2.h")


def test_splits_and_edges_of_the_shapes():
    assert D.splits(4097, 33, 256) == 2 and D.split_plan(4097, 33, 256) == (2, 2112)
    assert D.splits(9001, 33, 256) == 3 and D.split_plan(9001, 33, 256) == (3, 3008)
    assert 4097 - 2112 == 1985 and 9001 - 2 * 3008 == 2985
    assert D.splits(321, 96, 256) == 1
    for n in D.N_LIST:
        assert n % 64 != 0
        for m in D.M_LIST:
            assert D.splits(n, m, 256) == D.splits(n, m, 32) == -(-n // 4096)      # (any part with 32 CUs or more)
    assert 321 == D.tile(5) + 1 and all(321 > D.tile(k) for k in (6, 7, 8))
    assert D.last_tile(321, 33, 5) == (320, 321) and D.last_tile(4097, 33, 1) == (2112 + 1024, 4097)
    for k in D.K_ALL:                       # several SPA segments at every K, a ragged last one
        assert 9001 > 2 * D.spa_seg(k) and 9001 % D.spa_seg(k) != 0 and 4097 % D.spa_seg(k) == 1
    ks = {(n, m): sorted(k for (n2, m2, k) in D.SHAPES if (n2, m2) == (n, m)) for n in D.N_LIST for m in D.M_LIST}
    assert ks[(4097, 33)] == list(range(1, 17)) and all(v == [1, 3, 5, 8, 9, 16] for key, v in ks.items() if key != (4097, 33))
    assert len(D.SPA_CASES) == 20 and all(m == 96 for _, m, _ in D.SPA_CASES)


def _check_planted(n, m, k, kind, rows, valid, what):
    miss = D.as_oracle_rows(rows)
    miss = (rows == 0xFF) if rows.dtype == np.uint8 else np.isnan(miss)
    val = np.where(miss, 0, D.as_oracle_rows(rows)).astype(np.float64)
    P = D.PLANTED
    assert miss[P["all_missing"]].all() and not valid[P["all_missing"]], what
    assert not miss[P["all_zero"]].any() and (val[P["all_zero"]] == 0).all() and not valid[P["all_zero"]], what
    assert not miss[P["all_two"]].any() and (val[P["all_two"]] == 2).all() and not valid[P["all_two"]], what
    tail = n % 64
    r = P["tail_only"]
    assert not miss[r].any() and (val[r, :n - tail] == 0).all() and (val[r, n - tail:] > 0).all(), what
    assert bool(valid[r]) == (val[r].sum() >= 10), what                 # (N = 9001: 41 samples, a valid variant)
    r = P["missing_last_tile"]
    a, b = D.last_tile(n, m, k)
    assert miss[r].any() and not miss[r, :a].any() and miss[r, b - 1] and valid[r], what
    # the last sample is a call of 1 in several valid rows: a kernel that drops it moves their counts
    assert ((val[:, n - 1] > 0) & ~miss[:, n - 1] & (valid != 0)).sum() >= 3, what
    if kind == "u8":
        assert ((rows >= 3) & (rows < 0xFF)).sum() == 1, what
    elif kind == "i32":
        assert (rows == D.NONCALL_I32).sum() == 1 and (rows == D.NONCALL_U8).sum() == 1 and (rows == D.NA_INTEGER).any(), what
    else:
        assert (val != np.rint(val)).any() and np.nanmax(rows) <= 2.0, what


@pytest.mark.parametrize("n,m,k", BIG)
def test_cases_hold_what_they_name(n, m, k):
    for trait, spa_pval in (("quantitative", 0.05), ("binary", 0.05), ("binary", 0.0)):
        for kind in D.KINDS:
            what = f"N={n} M={m} K={k} {trait} spa_pval={spa_pval} {kind}"
            sm, rows = D.case(n, m, k, trait, kind, spa_pval=spa_pval)
            assert sm.k == k and sm.n == n and rows.shape == (m, n) and sm.spa_pval == spa_pval, what
            ref, valid, trace, _ = D.reference(n, m, k, trait, kind, spa_pval)
            v = valid.astype(bool)
            assert 2 * v.sum() >= m, f"{what}: {v.sum()} valid"
            assert (ref[v, 0] > 0.5).sum() >= 5, f"{what}: {(ref[v, 0] > 0.5).sum()} flipped"
            assert (~v).sum() >= 1, what
            assert np.isfinite(ref[v][:, :6]).all(), what
            _check_planted(n, m, k, kind, rows, valid, what)
            if trait == "binary":
                assert trace["flipped"] == (ref[v, 0] > 0.5).sum(), what
                if spa_pval == 0.0:
                    assert trace["spa_entered"] == 0 and trace["spa_done"] == 0, what
                else:
                    assert trace["spa_done"] >= 5, f"{what}: {trace}"


@pytest.mark.parametrize("n,m,k", [s for s in D.SHAPES if s[1] == 1])
def test_one_row_cases_are_valid(n, m, k):
    for trait in ("quantitative", "binary"):
        for kind in D.KINDS:
            _, valid, _, _ = D.reference(n, m, k, trait, kind, 0.0)
            assert valid.tolist() == [1], (n, k, trait, kind)


@pytest.mark.parametrize("n,m,k", D.SPA_CASES)
def test_flagged_count_of_the_spa_cases(n, m, k):
    """What test_gpu_ds_spa.py compares n_spa with: the variants that enter the saddlepoint approximation and do not
    leave at its first cutoff test."""
    for kind in ("u8", "f64"):
        ref, valid, trace, flagged = D.reference(n, m, k, "binary", kind, 0.05, True)
        assert flagged.sum() >= 5 and trace["spa_done"] >= 5, (n, k, kind, trace)
        assert flagged.sum() <= trace["spa_entered"] and not flagged[valid == 0].any()
        if trace["cutoff_doubled"] == 0:
            assert flagged.sum() == trace["spa_entered"] - trace["cutoff_exit"]
