"""The split flux item with the instruction forms of its FMA chains (profiles/flux_chain_ab.txt): sp_fast's magic
number in a vector register, exp2_fast's first Horner step and the thick branch's affine piece as one v_fma_f64 each, the Horner
steps inside one asm statement.  Every value keeps its operations and their operand order, so the fluxes keep their bits: forced
VAG_FLUX_SPLIT=2 against VAG_FLUX_SPLIT=0 on a persistent launch of wide workgroups, the form asserted from the launch report,
np.array_equal (the method and the helpers of tests/test_flux_split.py).

The ten bands from 1e9 to 1e18 Hz reach the thick term's and the nu_max term's exp2 (and every softplus term on its table side and
on both shortcut sides).  The new statements see different lane masks only at full and at partly filled boundary passes: lattices
of ~50, ~100 and ~200 nodes put 250 to 1000 work items on the 384 lanes of the boundary team, and the requested times 130 and 200
put one and two times on an interpolation lane.  The last case has the headline's lattice (>= 192 nodes at configs.C2's own
resolutions)."""
import numpy as np
import pytest

import configs
from test_flux_split import R5, R20, assert_bits, both, c2, eng, jittered  # noqa: F401  (eng: fixture)

pytestmark = pytest.mark.gpu
T = {nt: np.logspace(2, 8, nt) for nt in (130, 200)}


@pytest.fixture(scope="module")
def prms():
    return {"r5": c2(R5, 3, 310), "r20": c2(R20, 2, 311)}


@pytest.mark.parametrize("nt", [130, 200])
@pytest.mark.parametrize("g", ["r5", "r20"])
def test_chain_forms_keep_the_bits(eng, capfd, prms, g, nt):
    assert configs.C2_NU.size == 10 and configs.C2_NU.min() == 1e9 and configs.C2_NU.max() == 1e18
    assert_bits(*both(eng, capfd, prms[g], T[nt], configs.C2_NU))


def test_headline_lattice_keeps_the_bits(eng, capfd):
    p = jittered(configs.C2, 2, seed=312)
    assert_bits(*both(eng, capfd, p, T[200], configs.C2_NU))
