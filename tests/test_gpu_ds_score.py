"""The score stage on dosage rows, alone: every covariate count, sample split and tile edge of ds_scan_cases.py.

Dosage rows take score_ds_tile_kernel<P, T> + score_ds_tile_epilogue<P> (K <= 8) or score_ds_kernel<P, 256, T>
(K >= 9, and every K under "score_v1").  To keep the saddlepoint stage out of the comparison the models are
quantitative (launch_spa launches nothing) or binary with spa_pval = 0 (no variant is flagged: every SPA kernel leaves at
its empty-work check), so the table is the score stage's.  Against the CPU oracle; the oracle's tables are computed once
(ds_scan_cases.reference) and shared."""
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


def _case(n, m, k, trait, kind):
    sm, rows = D.case(n, m, k, trait, kind, spa_pval=0.0)
    ref, ref_valid, _, _ = D.reference(n, m, k, trait, kind, 0.0)
    return sm, rows, ref, ref_valid


@pytest.mark.parametrize("n,m,k,trait", D.SCORE_CASES)
def test_default_path_against_the_oracle(n, m, k, trait):
    """The shipped dispatch: the tiled kernels for K <= 8, the per-variant kernel for K >= 9; u8, f64 and i32 rows.  The
    same call twice on one handle gives the same bytes (the epilogue adds the splits in a fixed order)."""
    for kind in D.KINDS:
        sm, rows, ref, ref_valid = _case(n, m, k, trait, kind)
        with _scanner(sm) as sc:
            out, valid = D.scan(sc, rows)
            st = sc.stats()
            again, valid2 = D.scan(sc, rows)
        what = f"N={n} M={m} K={k} {trait} {kind}"
        assert st["n_variants"] == m and st["n_spa"] == 0 and st["n_valid"] == ref_valid.sum(), (what, st)
        assert st["score_launches"] == 1, f"{what}: the rows did not take the dosage kernels: {st}"
        D.check(out, valid, ref, ref_valid, n, kind, sm.quant, what)
        assert out.tobytes() == again.tobytes() and valid.tobytes() == valid2.tobytes(), f"{what}: two calls, two tables"


@pytest.mark.parametrize("n,m,k,trait", D.SCORE_CASES)
def test_score_v1_against_the_oracle_and_the_default_path(n, m, k, trait):
    """set_option("score_v1", 1): score_ds_kernel at every K -- for K <= 8 the only way it runs, for K >= 9 the kernel
    of the default path, so nothing may move there."""
    for kind in D.KINDS:
        sm, rows, ref, ref_valid = _case(n, m, k, trait, kind)
        with _scanner(sm) as sc:
            base, base_valid = D.scan(sc, rows)
            sc.set_option("score_v1", 1)
            out, valid = D.scan(sc, rows)
            st = sc.stats()
        what = f"N={n} M={m} K={k} {trait} {kind} score_v1"
        assert st["n_spa"] == 0 and st["score_launches"] == 1, (what, st)
        D.check(out, valid, ref, ref_valid, n, kind, sm.quant, what)
        assert np.array_equal(valid, base_valid), what
        v = ref_valid.astype(bool)
        np.testing.assert_allclose(out[v][:, 3:7], base[v][:, 3:7], rtol=1e-11, err_msg=what)
        if k >= 9:
            assert out.tobytes() == base.tobytes(), f"{what}: K >= 9 takes the same kernel either way"


def test_the_cases_have_more_than_one_split_on_this_device():
    """The split count depends on the number of compute units: on a part where the N = 4097 / 9001 cases fall back to
    one sample range the tests above would lose their multi-split coverage without a word."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for n, m, k, _ in D.SCORE_CASES:
        if n >= 4097:
            assert D.splits(n, m, n_cu) >= 2, (n, m, n_cu)
            assert D.split_plan(n, m, n_cu) == D.split_plan(n, m, D.N_CU), (n, m, n_cu)    # the planted last-tile row


@pytest.mark.parametrize("n,m,k,trait,kind", D.BLOCK_CASES)
def test_dosage_block_scan(n, m, k, trait, kind):
    """DosageBlock.load() / .scan(): the resident rows through the same kernels, the same table."""
    sm, rows, ref, ref_valid = _case(n, m, k, trait, kind)
    what = f"N={n} M={m} K={k} {trait} {kind} DosageBlock"
    with _scanner(sm) as sc, sc.dosage_block(rows.dtype, m) as blk:
        nv, _, _ = blk.load(rows)
        out, valid = blk.scan()
        st = sc.stats()
    miss = (rows == 0xFF) if kind == "u8" else np.isnan(rows)
    assert np.array_equal(nv, (~miss).sum(axis=1)), what
    assert st["n_spa"] == 0, (what, st)
    D.check(out, valid, ref, ref_valid, n, kind, sm.quant, what)
