"""Every shape of the contraction kernel and every branch of its work plan: score3_kernel is compiled for
NBF = 2..16 B fragments in a two-plane and a three-plane form (30 instantiations that differ in fragments per wave,
wave counts, ring depths and LDS size), and s3_plan cuts a call by tile groups, full rounds, leftover variant tiles
and pieces per leftover tile.  The cases of s3_cases.py (shown on the CPU, in test_s3_cases.py, to reach all of
that) are each scanned in both forms and held against the oracle at the 1e-10 rule and against each other: the
score stage's integers are the same in both forms, so validity, AF, mac and num agree to the bit and the other
columns to rounding.  The limb layout and the plan are recomputed from the device's own answers, so that a changed
limb rule or another CU count fails here instead of moving a case to another shape or branch."""
import numpy as np
import pytest

import s3_cases as S
from conftest import assert_table_close

# every test here needs the GPU; a hung kernel must fail the test, not stall the run
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """Import torch before the first HIP call of this process (libsaigehip.so binds to the torch wheel's runtime)."""
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


@pytest.fixture(scope="module")
def grid():
    """workgroups of the contraction kernel on this device, as host_scan.h counts them"""
    import torch
    return S.grid_of(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_shape_in_both_forms(c, grid):
    from oracle import Oracle
    from saigegds_amd._lib import Scanner
    M = S.variants(c, grid)                     # (c.M where the device has 256 CUs)
    got = S.reached(c, grid, M)
    assert c.branch in got, f"{c.name}: grid {grid}, M {M}: the plan takes {sorted(got)}"
    if c.m == "tile":
        assert ("f1-short" if c.branch == "f1-short" else "cut") in got, (c.name, grid, sorted(got))
    sm, packed = S.build(c, M)
    ref, ref_valid = Oracle(sm).scan_2bit(packed)
    v = ref_valid.astype(bool)
    assert 2 * v.sum() >= M and v[-16:].any()
    want = S.expected_limbs(sm)
    assert want.range_ok and want.nbf == c.nbf
    res = {}
    with Scanner(sm, device=0) as sc:
        limbs, ngroups = sc.score_layout()
        assert ngroups == 1 and np.array_equal(limbs, want.limbs), (c.name, limbs, want.limbs)
        for form in (1, 0):
            sc.set_option("three_plane", form)
            out, valid = sc.scan_2bit(packed)
            st = sc.stats()
            what = f"{c.name}: three_plane={form} NBF={c.nbf} N={c.n} M={M}"
            assert st["three_plane"] == form and st["score_launches"] > 0, (what, st)      # the fixed-point path ...
            if c.heavy:
                assert st["n_guarded"] < st["n_valid"], (what, st)
            else:
                assert st["n_guarded"] == 0, (what, st)                                     # ... for every variant
            assert_table_close(out, valid, ref, ref_valid, quant=sm.quant, what=what)
            res[form] = (out, valid)
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][0][v][:, :3], res[1][0][v][:, :3])
    cols = slice(3, 6) if sm.quant else slice(3, 7)
    np.testing.assert_allclose(res[0][0][v][:, cols], res[1][0][v][:, cols], rtol=1e-11)
