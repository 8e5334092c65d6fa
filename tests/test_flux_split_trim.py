"""The split form's boundary team evaluates its spectra with the thick-term bound (log2_I_nu_fast<true>: the optically thick
branch's softplus term is left out where the absorption blend drops the whole branch); the present kernel computes the term
everywhere.  Every (nu, t) sum must keep its bits: forced VAG_FLUX_SPLIT=2 against VAG_FLUX_SPLIT=0 on a persistent launch, the
form asserted from the launch report, a scramble call between, np.array_equal on finite, positive fluxes (the pattern and the
helpers of tests/test_flux_split.py).

The nt values walk the interpolation team's ownership of second times on both of its wavefronts (1, 8, 12, 13, 32, 33, 63 and
64 lanes of the last partly filled pass, and 64 / 128 times, where no lane owns two), at two lattice lengths.  Two cases put all
ten frequencies below the absorption break, where the term is needed, and far above it."""
import numpy as np
import pytest

import configs
from test_flux_split import NU, NU10, R5, R20, assert_bits, both, c2, eng  # noqa: F401  (eng: fixture)

pytestmark = pytest.mark.gpu

NT = [129, 136, 140, 141, 160, 161, 191, 192, 193, 200, 204, 205, 224, 225, 256, 64, 128]


@pytest.fixture(scope="module")
def prms():
    return {R20: c2(R20, 2, 81), R5: c2(R5, 2, 82)}


@pytest.mark.parametrize("res", [R20, R5], ids=["res20", "res5"])
@pytest.mark.parametrize("nt", NT)
def test_second_time_ownership_boundaries(eng, capfd, prms, nt, res):
    assert_bits(*both(eng, capfd, prms[res], np.logspace(2, 8, nt), NU10))


def test_three_frequencies_take_the_loop_form(eng, capfd, prms):
    assert_bits(*both(eng, capfd, prms[R20], np.logspace(2, 8, 200), NU[3]))


def test_late_window_leaves_rows_out(eng, capfd, prms):
    """Requested times from 3e7 s: the early rows of every model lie before the window (block-uniform skip on both teams)."""
    assert_bits(*both(eng, capfd, prms[R20], np.logspace(7.5, 8, 200), NU10))


@pytest.mark.parametrize("lo,hi", [(7, 9), (14, 18)], ids=["below_absorption_break", "far_above"])
def test_thick_term_needed_and_dropped(eng, capfd, prms, lo, hi):
    assert_bits(*both(eng, capfd, prms[R20], configs.C2_T, np.logspace(lo, hi, 10)))
