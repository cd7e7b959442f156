"""``seqAssocGLMM_spaSKAT`` / ``seqAssocGLMM_spaSKATO`` with ``collapse_mac`` on the device: 120 golden
variants (N = 1000) plus the constructed ultra-rare rows of tests/collapse_ref.py (1 to 10 minor alleles, some alt-major,
some with missing codes) in units of every shape.  The call with ``collapse_mac=10`` must equal, bit for bit on ``n.var``,
``Q``, every p-value column, ``rho.min`` and ``n.iter``, the same driver without the argument on a source that stores the
reference's pseudo-rows as real variants after all original rows, the units naming them last; ``n.collapsed`` and
``mac.collapsed`` are the reference's."""
import numpy as np
import pytest

from test_collapse_ref import check_against_stored

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_collapsed_call_equals_the_stored_pseudo_rows(test, trait):
    import saigegds_amd
    got = check_against_stored(getattr(saigegds_amd, "seqAssocGLMM_spa" + test), trait, None)
    print(test, trait, "n.var", got["n.var"].tolist(), "n.collapsed", got["n.collapsed"].tolist(),
          "mac.collapsed", got["mac.collapsed"].tolist())


@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_collapsed_call_with_grm_mat(test):
    import saigegds_amd
    import collapse_ref as CR
    from test_kmat_ds_ref import family
    ids = CR.driver_case("binary")[3]
    got = check_against_stored(getattr(saigegds_amd, "seqAssocGLMM_spa" + test), "binary", None, grm_mat=(ids, family()[0]))
    assert "n.iter" in got and got["n.iter"][[0, 1, 2, 3, 4, 6]].min() > 0 and got["n.iter"][5] == 0
