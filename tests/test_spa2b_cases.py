"""CPU: the case table of test_gpu_spa2b.py (spa2b_cases.py) reaches what it names -- by the oracle's count of flagged
variants and the carrier counts the library routes by: enough flagged variants on either side of SPA5_NNZ, both
orientations among them, several sample segments with a one-sample or ragged last one, and packed rows on the
intended side of the per-variant kernel's row-length thresholds.  Its copies of the library's constants are the
ones in the headers."""
import os

import numpy as np
import pytest

import spa2b_cases as S
from conftest import ROOT


def _src(name):
    return open(os.path.join(ROOT, "saigegds_amd", "csrc", name)).read()


def test_constants_are_the_headers():
    """A retuned threshold fails here instead of moving the code paths away from the cases unnoticed."""
    assert "#define SPA5_NNZ 8192 " in _src("dev_common.h") and S.SPA5_NNZ == 8192
    assert "if (nnz <= SPA5_NNZ) return (x <= SPA5_EXACT_X) ? 2 : 3;" in _src("dev_common.h")
    assert "h.minus ? (N - n2) : (n1 + n2 + n3), h.lut, pn, Ssc, v2sc, cbuf);" in _src("kern_score3.h")
    assert "const int full = row <= 32 ? 4096 : row <= 64 ? 2048 : row <= 128 ? 1024 : 512;" in _src("kern_spa2.h")
    host = _src("host_spa.h")
    assert "const size_t rowb5 = (size_t)((md.N + 63) / 64) * 16;" in host
    assert "const size_t l5 = (INPUT == IN_2BIT && rowb5 <= 120 * 1024) ? rowb5 : 0;" in host
    assert "const bool small5 = INPUT == IN_2BIT && rowb5 <= 32 * 1024;" in host
    assert "if (l5 > 48 * 1024 && !h->spa5_attr_set[INPUT]) {" in host
    assert "constexpr int UNG = K <= 4 ? 4 : 2;" in _src("kern_spa4.h")


def test_carriers_is_the_count_of_the_score_stage():
    c = np.array([0, 1, 2, 3, 0, 2, 2, 1], dtype=np.uint8)
    assert S.carriers(c, False) == 6 and S.carriers(c, True) == 5        # n1 + n2 + n3 = 2 + 3 + 1; N - n2 = 8 - 3


def test_segments_of_the_series_cases():
    assert sorted({S.spa_seg(k) for k in S.K_PER_SEG}) == [512, 1024, 2048, 4096]
    assert sorted(k for (n, _, k) in S.SERIES_CASES if n == S.N_SERIES) == list(range(1, 17))
    assert sorted(k for (n, _, k) in S.SERIES_CASES if n == 20011) == list(S.K_PER_SEG)
    for k in S.K_ALL:
        assert S.N_SERIES % S.spa_seg(k) == 1
    for n, m, k in S.SERIES_CASES + S.ROWLEN_CASES:
        assert n > 2 * S.spa_seg(k) and n % 64 != 0, (n, k)
    for k in S.K_PER_SEG:
        assert 20011 % S.spa_seg(k) > 1


def test_row_lengths_of_the_rowlen_cases():
    """(N + 63) / 64 * 16 bytes: 32 KiB < . <= 48 KiB -- 512 threads, staged, no attribute; 120 KiB < . -- not staged;
    each N is 64 x (pieces of the threshold row + 1) + 1: one sample in a second 16-byte piece past the threshold."""
    assert sorted({n for n, _, _ in S.ROWLEN_CASES}) == [S.N_STAGED_NO_ATTR, S.N_UNSTAGED]
    assert {k for _, _, k in S.ROWLEN_CASES} == {3, 9}
    b = S.row_bytes(S.N_STAGED_NO_ATTR)
    assert 32 * 1024 < b <= 48 * 1024 and b == 32 * 1024 + 32 and S.N_STAGED_NO_ATTR == 64 * (2048 + 1) + 1
    b = S.row_bytes(S.N_UNSTAGED)
    assert b > 120 * 1024 and b == 120 * 1024 + 32 and S.N_UNSTAGED == 64 * (7680 + 1) + 1


def _check_planted(n, m, k):
    c, _ = S.codes(n, m, k)
    ref, valid, _ = S.reference(n, m, k)
    P = S.PLANTED
    what = f"N={n} K={k}"
    assert (c[P["all_missing"]] == 3).all() and not valid[P["all_missing"]], what
    assert (c[P["all_zero"]] == 0).all() and not valid[P["all_zero"]], what
    assert (c[P["all_two"]] == 2).all() and not valid[P["all_two"]], what
    tail = n % 64
    r = c[P["tail_only"]]
    assert (r[:n - tail] == 0).all() and (r[n - tail:] == 2).all(), what
    assert bool(valid[P["tail_only"]]) == (2 * tail >= 10), what
    seg = S.spa_seg(k)
    a = (n - 1) // seg * seg
    r = c[P["missing_last_tile"]]
    assert (r == 3).any() and not (r[:a] == 3).any() and r[n - 1] == 3 and valid[P["missing_last_tile"]], what
    r = c[S.FIRST_SEG_ROW]
    assert (r[:seg] != 0).sum() > seg // 2 and (r[seg:n - 1] == 0).all() and r[n - 1] == 1 and valid[S.FIRST_SEG_ROW], what


@pytest.mark.parametrize("n,m,k", S.SERIES_CASES)
def test_series_cases_hold_what_they_name(n, m, k):
    sm, packed = S.case(n, m, k)
    assert sm.n == n and sm.k == k and sm.spa_pval == 0.05 and packed.shape == (m, (n + 3) // 4)
    g = S.flagged_groups(n, m, k)
    fl, many, flip = g["flagged"], g["many"], g["flip"]
    counts = {"flagged": int(fl.sum()), "over 8192 carriers": int((fl & many).sum()), "of them alt-major": int((fl & many & flip).sum()),
              "at most 8192": int((fl & ~many).sum()), "of them alt-major ": int((fl & ~many & flip).sum())}
    print(f"N={n} M={m} K={k}: {counts}")
    assert (fl & many).sum() >= 8, counts
    assert (fl & ~many).sum() >= 5, counts
    assert (fl & many & flip).sum() >= 1 and (fl & ~many & flip).sum() >= 1, counts
    assert not fl[S.reference(n, m, k)[1] == 0].any()
    _check_planted(n, m, k)


@pytest.mark.parametrize("n,m,k", S.ROWLEN_CASES)
def test_rowlen_cases_hold_what_they_name(n, m, k):
    sm, packed = S.case(n, m, k)
    assert sm.n == n and sm.k == k and packed.shape == (m, (n + 3) // 4)
    g = S.flagged_groups(n, m, k)
    fl, many, flip = g["flagged"], g["many"], g["flip"]
    counts = {"flagged": int(fl.sum()), "over 8192 carriers": int((fl & many).sum()), "at most 8192": int((fl & ~many).sum()),
              "of them alt-major": int((fl & ~many & flip).sum())}
    print(f"N={n} M={m} K={k}: {counts}")
    assert (fl & ~many).sum() >= 5, counts
    _check_planted(n, m, k)
