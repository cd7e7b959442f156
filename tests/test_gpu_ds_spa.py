"""The saddlepoint stage on dosage rows at every covariate count: binary cases of ds_scan_cases.py with the default
spa_pval = 0.05, so that the flagged variants go through spa4_moments_ds<K, NC, INPUT> (segments of spa_seg(K) samples,
both tiers), spa4_solve and the IN_U8 / IN_F64 forms of the per-variant kernels -- or, under "score_v1", through
spa_kernel<K, 512, INPUT> alone.  Full rows against the CPU oracle; the score stage on its own is
test_gpu_ds_score.py's.  Dosage rows always start in tier A; 2-bit rows are routed by their carrier count and reach
the cumulant pass only with more than 8192 carriers: see test_gpu_spa2b.py."""
import numpy as np
import pytest

import ds_scan_cases as D

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _scanner(sm):
    from saigegds_amd._lib import Scanner
    return Scanner(sm, device=0)


def _case(n, m, k, kind):
    sm, rows = D.case(n, m, k, "binary", kind)
    ref, ref_valid, trace, flagged = D.reference(n, m, k, "binary", kind, 0.05, True)
    return sm, rows, ref, ref_valid, int(flagged.sum())


@pytest.mark.parametrize("n,m,k", D.SPA_CASES)
def test_series_stage_against_the_oracle(n, m, k):
    for kind in ("u8", "f64"):
        sm, rows, ref, ref_valid, nflag = _case(n, m, k, kind)
        with _scanner(sm) as sc:
            out, valid = D.scan(sc, rows)
            st = sc.stats()
        what = f"N={n} M={m} K={k} binary {kind}"
        print(f"{what}: n_spa {st['n_spa']} (oracle {nflag}), exact sweeps {st['n_spa_slow']}, dense {st['n_spa_dense']}")
        D.check(out, valid, ref, ref_valid, n, kind, False, what)
        assert st["n_spa"] == nflag and nflag >= 5, (what, st, nflag)
        # (strong signals go on to the exact sweeps; what the series itself answers has to be part of the comparison)
        assert st["n_spa"] - st["n_spa_slow"] - st["n_spa_dense"] >= 5, (what, st)


@pytest.mark.parametrize("option", ["score_v1", "spa_exact"])
@pytest.mark.parametrize("k", D.SPA_PATH_K)
def test_other_spa_routes_against_the_oracle(k, option):
    """The same rows with every flagged variant through spa_kernel ("score_v1") or through the exact exp / log sweeps
    ("spa_exact"), as test_fallback_paths_give_identical_rows does for 2-bit rows."""
    n, m = 4097, 96
    for kind in ("u8", "f64"):
        sm, rows, ref, ref_valid, nflag = _case(n, m, k, kind)
        with _scanner(sm) as sc:
            base, _ = D.scan(sc, rows)
            sc.set_option(option, 1)
            out, valid = D.scan(sc, rows)
            st = sc.stats()
        what = f"N={n} M={m} K={k} binary {kind} {option}"
        D.check(out, valid, ref, ref_valid, n, kind, False, what)
        assert st["n_spa"] == nflag, (what, st, nflag)
        if option == "spa_exact":               # the exact sweeps, or the exact dense pass where the g_pos / g_neg test sends a variant
            assert st["n_spa_slow"] >= 1 and st["n_spa_slow"] + st["n_spa_dense"] == nflag, (what, st)
        v = ref_valid.astype(bool)
        np.testing.assert_allclose(out[v][:, 3:7], base[v][:, 3:7], rtol=1e-11, err_msg=what)
