"""CPU: the case table of test_gpu_score3_shapes.py (s3_cases.py) reaches what it says it reaches -- every one of
the 30 (form, NBF) shapes of score3_kernel and every branch of s3_plan -- its copy of the shape tables is the one in
kern_score3.h, and every case gives the GPU test something to compare: valid variants up to the last fragment,
missing genotypes among them, flipped variants."""
import functools
import os
import re

import numpy as np
import pytest

import s3_cases as S
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def _model(name):
    (c,) = [c for c in S.CASES if c.name == name]
    return S.build_model(c)


def _header_table(macro):
    """the entries X(...) of a `#define macro(X) \\` ... in kern_score3.h, as tuples of ints"""
    text = open(os.path.join(ROOT, "saigegds_amd", "csrc", "kern_score3.h")).read()
    m = re.search(r"^#define " + macro + r"\(X\)((?:.*\\\n)*.*)$", text, re.M)
    assert m, macro
    return [tuple(int(v) for v in e.split(",")) for e in re.findall(r"X\(([^)]*)\)", m.group(1))]


def test_shape_tables_are_the_headers():
    """A retuned table fails here instead of moving the cases to other variant counts unnoticed."""
    for form, macro in S.SHAPE_MACRO.items():
        got = _header_table(macro)
        assert [s[0] for s in got] == list(range(2, 17)), macro
        assert got == S.SHAPES[form], macro


def test_plan_on_worked_examples():
    """s3_plan by hand: the numbers of s3_layout.h's own rule on four rows of the table."""
    p = S.plan(2117, 16_411, 256, 1, 11)            # 66 tiles in 8 groups of 32 workgroups; 133 fragments in tiles of 4
    assert (p.ntile, p.ng, p.wpg, p.nfrag, p.vt, p.rf, p.rem, p.f, p.ipg) == (66, 8, 32, 133, 34, 1, 2, 2, 36)
    p = S.plan(2048, 16_411, 256, 1, 11)
    assert (p.vt, p.rf, p.rem, p.f, p.ipg) == (32, 1, 0, 0, 32)
    p = S.plan(1280, 16_411, 256, 1, 11)            # 20 leftover tiles on 32 workgroups: not cut
    assert (p.vt, p.rf, p.rem, p.f, p.ipg) == (20, 0, 20, 1, 20)
    p = S.plan(529, 3001, 256, 0, 3)                # 12 tiles: one group, pieces of at least 4 tiles
    assert (p.ntile, p.ng, p.wpg, p.vt, p.rf, p.rem, p.f) == (12, 1, 256, 2, 0, 2, 3)
    assert [S.plan(1, n, 256, 0, 4).ng for n in (700, 3001, 5000, 9001, 16_411)] == [1, 1, 2, 4, 8]
    assert [S.ntile_of(n) for n in (700, 3001, 5000, 9001, 16_411)] == [4, 12, 20, 36, 66]


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_case_has_its_shape_and_branch(c):
    e = S.expected_limbs(_model(c.name))
    assert e.range_ok and e.nbf == c.nbf, (c.name, e)
    assert (e.limbs[:c.k] == 0).all() == (c.trait == "quantitative")        # the synthetic quantitative models derive c'
    assert S.variants(c) == c.M
    got = S.reached(c)
    assert c.branch in got, (c.name, got)
    if c.m == "tile":
        assert c.M == 16 * max(S.fpw(0, c.nbf), S.fpw(1, c.nbf)) + 17
        assert ("f1-short" if c.branch == "f1-short" else "cut") in got, (c.name, got)     # pieces in both forms
        for form in (0, 1):                     # a full variant tile and a ragged one
            p = S.plan(c.M, c.n, 256, form, c.nbf)
            assert p.rf == 0 and p.rem == p.vt >= 2 and c.M % 16 == 1
    if c.heavy:
        plain = 2 * c.k * S.MF_NLIMB - c.k + 2 * S.MF_NLIMB + 1             # K = 16, N < 16 384: 6-limb c', 7 elsewhere
        assert c.n < 16384 and e.used >= plain + 2 and (e.limbs[:c.k] == S.MF_NLIMB).sum() >= 2


def test_table_reaches_every_shape_and_branch():
    nbfs = {c.nbf for c in S.CASES}
    assert {(form, nbf) for form in (0, 1) for nbf in nbfs} == {(form, s[0]) for form in (0, 1) for s in S.SHAPES[form]}
    assert len(S.SHAPES[0]) == len(S.SHAPES[1]) == 15
    small = {c.nbf for c in S.CASES if c.n == S.N_S and c.m == "tile"}
    assert small == set(range(2, 17))                                        # every NBF on one full and one ragged tile
    large = {c.nbf for c in S.CASES if c.n >= 16384 and c.k not in (3, 5)}
    assert len(large) >= 4, large
    seen = set().union(*(S.reached(c) for c in S.CASES))
    assert S.BRANCHES <= seen, S.BRANCHES - seen
    assert {c.branch for c in S.CASES} | {"cut"} == S.BRANCHES
    assert len({c.name for c in S.CASES}) == len(S.CASES) and len({c.seed for c in S.CASES}) == len(S.CASES)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_oracle_table_has_something_to_compare(c):
    """The GPU test must not pass on nothing: from the oracle alone, at least half of the variants are valid, one
    of the last 16 is (the ragged fragment), valid rows hold missing genotypes (the third plane / the lists carry
    data) and at least 10 valid variants are flipped."""
    from oracle import Oracle
    from saigegds_amd.gds import unpack_dosage_2bit
    sm, packed = _model(c.name), S.build_rows(c)
    assert packed.shape[0] == c.M
    orc = Oracle(sm)
    ref, valid = orc.scan_2bit(packed)
    v = valid.astype(bool)
    assert 2 * v.sum() >= c.M, (c.name, int(v.sum()))
    assert v[-16:].any()
    assert (unpack_dosage_2bit(packed[v], c.n) == 3).any()
    flipped = int((ref[v][:, 0] > 0.5).sum())
    if not sm.quant:                            # (the oracle traces its binary branch only)
        assert orc.trace.as_dict()["flipped"] == flipped
    assert flipped >= 10, (c.name, flipped)
