"""The split form's boundary team evaluates the two frequencies of a work item with softplus terms of one masked region each
(log2_I_nu_fast<true, true>: sp_fast<RELU_FIRST>, vag_device.h) -- or, in a -DVAG_FLUX_PAIR build, with log2_I_nu_pair, which
requests the table rows of independent softplus terms together (measured and not taken: profiles/flux_prefetch_ab.txt).  The plain
kernel makes two single calls per item with the plain softplus.  Every (nu, t) sum must keep its bits: forced VAG_FLUX_SPLIT=2
against VAG_FLUX_SPLIT=0 on a persistent launch of wide workgroups, the form asserted from the launch report, a scramble call between, np.array_equal on finite
fluxes (the pattern and the helpers of tests/test_flux_split.py).

Small cases where a boundary item's evaluation can go wrong: lattices of ~100 and ~200 nodes, two models, 37 times; ten
frequencies and three (odd: the duplicated last pair, both frequencies of the last item the same); all frequencies below the absorption break (the thick
term needed in most lanes) and far above it (every break shortcut taken); a set that straddles nu_max (the cut taken by one
frequency of an item and not by the other, and by some lattice nodes only); a late window (few window nodes: a pass with mostly idle
lanes); one row per item."""
import numpy as np
import pytest

from test_flux_split import NU, NU10, R5, R10, assert_bits, both, c2, eng  # noqa: F401  (eng: fixture)

pytestmark = pytest.mark.gpu

T37 = np.logspace(2.5, 7.5, 37)
SETS = {
    "ten": NU10,
    "three": NU[3],
    "below_absorption_break": np.logspace(7, 9, 10),
    "far_above": np.logspace(14, 18, 10),
    "across_nu_max": np.logspace(18, 28, 10),
}


@pytest.fixture(scope="module")
def prms():
    return {R5: c2(R5, 2, 91), R10: c2(R10, 2, 92)}


@pytest.mark.parametrize("res", [R5, R10], ids=["res5", "res10"])
@pytest.mark.parametrize("nu", list(SETS), ids=list(SETS))
def test_frequency_sets(eng, capfd, prms, nu, res):
    new, old = both(eng, capfd, prms[res], T37, SETS[nu])
    assert_bits(new, old)
    if nu == "across_nu_max":  # the lowest frequency lies below the cut, the highest is cut away
        assert new[:, 0].min() > 0 and new[:, -1].max() < 1e-30 * new[:, 0].max()


@pytest.mark.parametrize("res", [R5, R10], ids=["res5", "res10"])
def test_late_window_few_nodes_per_pass(eng, capfd, prms, res):
    assert_bits(*both(eng, capfd, prms[res], np.logspace(7.5, 8, 37), NU10))


@pytest.mark.parametrize("res", [R5, R10], ids=["res5", "res10"])
def test_one_row_per_item(eng, capfd, prms, res):
    assert_bits(*both(eng, capfd, prms[res], T37, NU10, {"VAG_PAIRS_PER_BLOCK": "1"}))
