"""The split flux item at the places where a row's header -- the window nodes, the count of work items, the steps of a lane's walk,
whether the row is skipped -- or an item's start can go wrong (profiles/flux_header_ab.txt).  That record built a
row header formed once per row by the EAT wavefronts and handed to the boundary team through LDS, measured it (+1.75 % per step)
and took it out; it kept the item's start without the LDS copy of the requested times and its barrier, the item number in an LDS
word of its own, and the softplus terms' table side ending in r + p.  These cases were written for the header and hold whichever
form is built.  No sum, addend or order changes: forced VAG_FLUX_SPLIT=2 against VAG_FLUX_SPLIT=0 on a persistent launch of wide
workgroups, the form asserted from the launch report, np.array_equal (the method and the helpers of tests/test_flux_split.py and
tests/test_flux_split_prologue.py).

Items of one, two and three rows and a last item of one row (the pipeline fills and drains, both parity slots are written before
either is read; an item of one row starts staging while a slower wavefront still reads the item's number); an on-axis model (every
row's EAT step runs behind a re-staging); windows of early and late requested times (skipped rows between used ones, n_lt = 0,
n_le = K, both clamps of k_lo / k_hi) and a narrow one inside the light curve (nk changes from row to row); lattices of ~50, ~100
and ~200 nodes (nk crosses the multiples of 64, the work items cross one and two passes of the 384 lanes); one call mixing
resolutions with fewer workgroups than items (a workgroup meets another K and n_phi, the representative row at the phi wrap of
each, and the next item's number); a rejected model in the middle; the same call twice.  Ten frequencies, 130 and 200 times, at
most four models."""
import re

import numpy as np
import pytest

import _abi
import configs
from test_flux_split import M12, NU10, R5, R10, R20, assert_bits, both, c2, eng, run_form  # noqa: F401  (eng: fixture)
from test_flux_split_prologue import last_item_of_one_row, ppb

gpu = pytest.mark.gpu
GRIDS = {"m12": M12, "r5": R5, "r10": R10, "r20": R20}
T = {130: np.logspace(2.5, 7.5, 130), 200: np.logspace(2.5, 7.5, 200)}
WINDOWS = {"late": np.logspace(7.5, 8, 130), "early": np.logspace(0, 1.5, 130), "narrow": np.logspace(4.5, 5.5, 200)}


@pytest.fixture(scope="module")
def prms():
    return {k: c2(res, 2, 210 + i) for i, (k, res) in enumerate(GRIDS.items())}


def items_of(report, n_models):
    m = re.search(r"grid flux form: persistent, (\d+) workgroups for (\d+) items", report)
    assert m, report
    assert int(m.group(2)) % n_models == 0
    return int(m.group(1)), int(m.group(2)) // n_models


@gpu
@pytest.mark.parametrize("g,nt", [("m12", 200), ("r10", 130), ("r20", 200)])
@pytest.mark.parametrize("rows_per_item", [1, 2, 3, "last_of_one"])
def test_fill_drain_and_the_parity_slots(eng, capfd, prms, rows_per_item, g, nt):
    n = rows_per_item
    if rows_per_item == "last_of_one":
        # rows of the batch's largest model: the items of a launch of one row per item, over the models
        _, rows = items_of(run_form(eng, capfd, 2, prms[g], T[130][:9], NU10, ppb(1))[2], len(prms[g]))
        n = last_item_of_one_row(rows)
        assert n >= 4 and rows % n == 1
    assert_bits(*both(eng, capfd, prms[g], T[nt], NU10, ppb(n)))


@gpu
@pytest.mark.parametrize("rows_per_item", [1, 2, 7])
def test_on_axis_every_row_follows_a_restaging(eng, capfd, rows_per_item):
    assert_bits(*both(eng, capfd, c2(R10, 3, 220, theta_obs=0.0), T[130], NU10, ppb(rows_per_item)))


@gpu
@pytest.mark.parametrize("g", ["r5", "r10", "r20"])
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("rows_per_item", [3, 50])
def test_windows_that_skip_rows_and_clamp_the_nodes(eng, capfd, prms, g, window, rows_per_item):
    """Late times: the rows near the axis end before the window opens (n_lt = K, skipped) and the rows behind them do not.  Early
    times: the window closes before most nodes (n_le small, k_hi clamped from below, n_lt = 0).  Narrow: nk changes with the row."""
    new, old = both(eng, capfd, prms[g], WINDOWS[window], NU10, ppb(rows_per_item))
    assert_bits(new, old)


@gpu
@pytest.mark.parametrize("g", ["r5", "r10", "r20"])
def test_lattices_of_50_100_and_200_nodes(eng, capfd, prms, g):
    assert_bits(*both(eng, capfd, prms[g], T[200], NU10, ppb(50)))


@gpu
@pytest.mark.parametrize("rows_per_item", [2, 3])
def test_one_workgroup_meets_another_lattice_and_phi_wrap(eng, capfd, rows_per_item):
    p = c2(R10, 1, 230) + c2(M12, 1, 231) + c2(R20, 1, 232) + c2(R5, 1, 233)
    new, _, report = run_form(eng, capfd, 2, p, T[200], NU10, ppb(rows_per_item))
    m = re.search(r"grid flux form: persistent, (\d+) workgroups for (\d+) items", report)
    assert m and int(m.group(1)) < int(m.group(2)), report  # a workgroup takes more than one item
    old = run_form(eng, capfd, 0, p, T[200], NU10, ppb(rows_per_item))[0]
    assert_bits(new, old)


@gpu
def test_rejected_model_in_the_middle(eng, capfd):
    p = c2(R10, 1, 240) + c2(M12, 1, 241) + c2(R10, 1, 242)
    p.insert(1, _abi.make_params(**dict(configs.C2, resolutions=(200.0, 0.31, 5.0))))  # beyond the grid kernel's layouts: status != 0
    cap = {rc for rc in range(-64, 65) if rc != 0}  # the call reports the rejected model after it has written the others
    new, rc_new, _ = run_form(eng, capfd, 2, p, T[130], NU10, ppb(3), ok_rc=cap)
    old, rc_old, _ = run_form(eng, capfd, 0, p, T[130], NU10, ppb(3), ok_rc=cap)
    assert rc_new == rc_old and rc_new != 0
    assert_bits(new[[0, 2, 3]], old[[0, 2, 3]])


@gpu
def test_same_call_twice_gives_the_same_bits(eng, capfd, prms):
    a = run_form(eng, capfd, 2, prms["r10"], T[200], NU10, ppb(3))[0]
    b = run_form(eng, capfd, 2, prms["r10"], T[200], NU10, ppb(3))[0]
    old = run_form(eng, capfd, 0, prms["r10"], T[200], NU10, ppb(3))[0]
    assert_bits(a, b)
    assert_bits(a, old)
