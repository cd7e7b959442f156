"""CPU: the yardsticks of the explicit-GRM tests (grm_dense_ref.py).  E_DENSE is re-measured -- a plain float64
g.T @ g / M against the long-double reference over every shape of the GPU tests -- and must not be exceeded; and no
reference entry of a planted case lies within 1e-9 of a cutoff the GPU tests use, so that their set comparison
needs no exclusions."""
import numpy as np
import pytest

import grm_dense_ref as D
import grm_ref as R


def test_exact_gram_matches_a_long_double_loop():
    codes = R.make_codes(23, 131, 5, 0.05)
    g = D._g(codes, -1)
    want = np.zeros((23, 23), dtype=D.LD)
    for v in range(g.shape[0]):
        want += np.outer(g[v], g[v])
    got = D._gram_exact(g)
    assert float(np.max(np.abs(got - want))) <= 131 * 2.0 ** -63 * float(np.max(np.abs(want)))


_worst = {}


@pytest.mark.parametrize("c", D.CASES + [(n, m, 5e-3) for n, m in D.PLANTED], ids=R.case_id)
def test_double_gram_stays_within_e_dense(c):
    n, m, miss = c
    if (n, m) in D.PLANTED:
        p, ref = D.planted(n, m)
        codes = p.codes
    else:
        codes, ref = D.case(n, m, miss)
    e = D.scaled_error(D.double_gram(codes), ref)
    _worst[c] = e
    print("\n%s scaled error %.4g (worst so far %.4g)" % (R.case_id(c), e, max(_worst.values())))
    assert e <= D.E_DENSE
    assert np.all(ref.K[:, n - 1] == 0) and np.all(ref.K[n - 1] == 0)      # the all-missing sample: a zero row


@pytest.mark.parametrize("n,m", D.PLANTED)
def test_planted_relatives_stand_clear_of_every_cutoff(n, m):
    p, ref = D.planted(n, m)
    K = ref.K
    for c in D.CUTOFFS:
        assert float(np.min(np.abs(K - D.LD(c)))) > 1e-9, c
    assert abs(float(K[p.dup]) - float(K[p.dup[0], p.dup[0]])) < 1e-12 and float(K[p.dup]) > 0.4
    for a, b in p.parent_child + [p.sibs]:
        assert float(K[a, b]) > 0.25, (a, b, float(K[a, b]))
    assert K[p.disjoint] == 0 and ref.scale[p.disjoint] == 0
    iu = np.triu_indices(n, 1)
    assert float(np.median(np.abs(K[iu]))) < 0.05                      # and the bulk lies well below 0.125
