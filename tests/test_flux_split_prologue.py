"""What a wavefront of the split flux item does between a row's barrier and its first work item was shortened (DESIGN 4g item 11,
profiles/flux_prologue_ab.txt): the boundary team reads the row header -- the ends of the row's lattice and the window words of the
EAT wavefronts -- in one LDS round trip, the window of the requested times is a constant of the item held in registers, and the step
of the boundary items AL / nk comes from the loop's reciprocal (flux_quot_adjust, vag_flux_limits.h).  The same record measured and
rejected forms that CARRY values from one row's interval to the next (the representative row, the row's solid angle, cos_v and
t_coeff of the EAT wavefronts' next row, requested with scalar loads an interval ahead).  No sum, addend or order changes in any of
them: forced VAG_FLUX_SPLIT=2 against VAG_FLUX_SPLIT=0 on a persistent launch of wide workgroups, the form asserted from the
launch report, np.array_equal (the method and the helpers of tests/test_flux_split.py).

The cases are the places where a value kept across rows or items can go stale, whichever form is built: items of one, two and three
rows and a last item of one row (the pipeline fills and drains; a row past the item must not be read); an on-axis model (the staged
block changes at every row, the EAT step of every row runs behind the re-staging); a window that leaves a model's early rows out
(skipped rows between used ones); one call whose models differ in resolution, with fewer workgroups than items (a workgroup goes
from an item of one n_phi and K to one of another); a rejected model in the
middle; the same call twice.  Small grids, ten frequencies, 130 and 200 times, at most four models.

The quotient is checked on the host (tests/flux_quot_check.cpp), without a device."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import _abi
import configs
from test_flux_split import M12, NU10, R5, R10, assert_bits, both, c2, eng, grid, run_form  # noqa: F401  (eng: fixture)
from vegasafterglow_amd import _lib

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"m12": M12, "r5": R5}
T = {130: np.logspace(2.5, 7.5, 130), 200: np.logspace(2.5, 7.5, 200)}


def ppb(n):
    return {"VAG_PAIRS_PER_BLOCK": str(n)}


@pytest.fixture(scope="module")
def prms():
    return {k: c2(res, 2, 110 + i) for i, (k, res) in enumerate(GRIDS.items())}


@pytest.fixture(scope="module")
def rows(eng, prms):
    """Rows (theta, phi pairs) of the batch's largest model, per grid: the items of a launch of one row per item, over the models.
    (capfd is function-scoped: the launch report is taken from file descriptor 2, as b_lanes of tests/test_flux_split.py does.)"""
    hooks = {"VAG_DEBUG_LAUNCH": "1", "VAG_FLUX_WIDE": "1", "VAG_FLUX_PERSISTENT": "2", "VAG_FLUX_SPLIT": "2", **ppb(1)}
    out = {}
    for k, p in prms.items():
        saved = os.dup(2)
        with tempfile.TemporaryFile() as f:
            os.dup2(f.fileno(), 2)
            for h, v in hooks.items():
                _lib.hooks[h] = v
            try:
                grid(eng, p, T[130][:9], NU10)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                for h in hooks:
                    _lib.hooks.pop(h, None)
            f.seek(0)
            err = f.read().decode()
        m = re.search(r"grid flux form: persistent, \d+ workgroups for (\d+) items", err)
        assert m, err
        assert int(m.group(1)) % len(p) == 0
        out[k] = int(m.group(1)) // len(p)
    return out


def last_item_of_one_row(n_rows):
    """Rows per item that leave the largest model a last item of ONE row: the smallest divisor >= 4 of n_rows - 1."""
    return next(d for d in range(4, n_rows) if (n_rows - 1) % d == 0)


@gpu
@pytest.mark.parametrize("nt", [130, 200])
@pytest.mark.parametrize("g", list(GRIDS))
@pytest.mark.parametrize("rows_per_item", [1, 2, 3, "last_of_one"])
def test_fill_drain_and_the_held_request(eng, capfd, prms, rows, rows_per_item, g, nt):
    n = last_item_of_one_row(rows[g]) if rows_per_item == "last_of_one" else rows_per_item
    if rows_per_item == "last_of_one":
        assert n >= 4 and rows[g] % n == 1
    assert_bits(*both(eng, capfd, prms[g], T[nt], NU10, ppb(n)))


@gpu
@pytest.mark.parametrize("rows_per_item", [1, 2, 3, 7])
def test_on_axis_the_staged_block_changes_at_every_row(eng, capfd, rows_per_item):
    assert_bits(*both(eng, capfd, c2(R5, 3, 120, theta_obs=0.0), T[130], NU10, ppb(rows_per_item)))


@gpu
@pytest.mark.parametrize("g", list(GRIDS))
@pytest.mark.parametrize("rows_per_item", [3, 50])
def test_window_that_leaves_the_early_rows_out(eng, capfd, prms, g, rows_per_item):
    """Late requested times: the rows near the axis end before the window opens and are skipped by both teams (the header read says
    so), the rows behind them are not."""
    new, old = both(eng, capfd, prms[g], np.logspace(7.5, 8, 130), NU10, ppb(rows_per_item))
    assert_bits(new, old)


@gpu
@pytest.mark.parametrize("rows_per_item", [1, 2, 3])
def test_one_workgroup_takes_items_of_different_resolutions(eng, capfd, rows_per_item):
    p = c2(M12, 1, 130) + c2(R5, 1, 131) + c2(R10, 1, 132) + c2(M12, 1, 133)
    new, _, report = run_form(eng, capfd, 2, p, T[200], NU10, ppb(rows_per_item))
    m = re.search(r"grid flux form: persistent, (\d+) workgroups for (\d+) items", report)
    assert m and int(m.group(1)) < int(m.group(2)), report  # a workgroup takes more than one item
    old = run_form(eng, capfd, 0, p, T[200], NU10, ppb(rows_per_item))[0]
    assert_bits(new, old)


@gpu
def test_rejected_model_in_the_middle(eng, capfd):
    p = c2(M12, 1, 140) + c2(R5, 1, 141) + c2(M12, 1, 142)
    p.insert(1, _abi.make_params(**dict(configs.C2, resolutions=(200.0, 0.31, 5.0))))  # beyond the grid kernel's layouts: status != 0
    cap = {rc for rc in range(-64, 65) if rc != 0}  # the call reports the rejected model after it has written the others
    new, rc_new, _ = run_form(eng, capfd, 2, p, T[130], NU10, ppb(2), ok_rc=cap)
    old, rc_old, _ = run_form(eng, capfd, 0, p, T[130], NU10, ppb(2), ok_rc=cap)
    assert rc_new == rc_old and rc_new != 0
    assert_bits(new[[0, 2, 3]], old[[0, 2, 3]])


@gpu
def test_same_call_twice_gives_the_same_bits(eng, capfd, prms):
    a = run_form(eng, capfd, 2, prms["r5"], T[200], NU10, ppb(3))[0]
    b = run_form(eng, capfd, 2, prms["r5"], T[200], NU10, ppb(3))[0]
    assert_bits(a, b)


def test_quotient_from_the_reciprocal_on_the_host(tmp_path):
    """AL / nk for AL = 384 and every nk in 1 .. 204, the reciprocal moved by up to four units in the last place (no device)."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found: the check of flux_quot_adjust needs one")
    exe = tmp_path / "flux_quot_check"
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "flux_quot_check.cpp"), "-o", str(exe)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and ran.stdout.startswith("ok flux_quot_adjust"), ran.stdout
