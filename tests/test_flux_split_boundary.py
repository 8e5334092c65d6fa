"""What a workgroup of the split flux kernel does BETWEEN rows was changed (profiles/flux_boundary_ab.txt): the
photon block is staged in one round trip to HBM, every lane requesting all its words before it stores the first, with (parameter,
node) advanced by a carry (stage_photon_block_split).  The same record measured and removed other forms of the hand-over between
items and of the row behind a staging (its EAT step from the block in HBM beside the staging; no LDS copy of the requested times,
the item number in an LDS word of its own and a barrier less at the item's start).  No sum, addend or order changes in any of
them: forced VAG_FLUX_SPLIT=2 against VAG_FLUX_SPLIT=0 on a persistent launch of wide workgroups, the form asserted from the launch
report, np.array_equal (the method and the helpers of tests/test_flux_split.py).

The cases are the places where the hand-over between items and the staging can go wrong, whichever form is built: one batch of
four redshifts cut into thousands of items (every workgroup takes many items in a row and changes model, so the frequencies in LDS
and the item word are rewritten under way); lattice lengths either side of what the staging steps over (18 K words dealt over 512
lanes: 18 K just below and just above a multiple of 512, K < 64, 64 < K < 128, K > 128, the headline's 199 and the longest lattice
the split form accepts at ten frequencies and 200 times, with the next one refused); an on-axis model (every row stages); items
that end on, straddle and follow the change of the photon block; a rejected model among items of one row; and fewer items than
resident workgroups, called twice with a call of another shape between.  Small grids, ten frequencies, at most thirteen models."""
import ctypes as C
import re

import numpy as np
import pytest

import _abi
import configs
from test_flux_split import M12, NU10, R5, R10, R20, assert_bits, both, c2, eng, grid, run_form  # noqa: F401  (eng: fixture)
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
T37 = np.logspace(2.5, 7.5, 37)
LANES, NPAR = 512, 18  # lanes of a workgroup, members of a staged node (VAG_NPAR): the staging deals NPAR * K words over LANES


def ppb(n):
    return {"VAG_PAIRS_PER_BLOCK": str(n)}


def plain(res, **kw):
    """configs.C2 at resolution `res`, not jittered: the lattice length is then the one the cases below name."""
    return _abi.make_params(**dict(configs.C2, resolutions=res, **kw))


def report_of(err):
    m = re.search(r"grid flux form: persistent, (\d+) workgroups for (\d+) items", err)
    k = re.search(r"grid flux launch: .* ks=(\d+) ", err)
    assert m and k, err
    return int(m.group(1)), int(m.group(2)), int(k.group(1))


def both_reported(eng, capfd, prms, t, nu, extra=None, **kw):
    """both() of tests/test_flux_split.py, with the split call's (workgroups, items, K) from its launch report."""
    new = run_form(eng, capfd, 2, prms, t, nu, extra, **kw)
    old = run_form(eng, capfd, 0, prms, t, nu, extra, **kw)
    return new[0], old[0], report_of(new[2])


def n_phi_eff_of(eng, prm, t):
    """Phi rows per theta row of the model's grid, as the library reports it (vag_details_eat)."""
    lib, h = eng
    p = _lib.ModelParams.from_buffer_copy(bytes(prm))
    npe = C.c_int(0)
    _lib.check(lib.vag_details_eat(h, C.byref(p), float(t[0]), float(t[-1]), C.byref(npe), None, None))
    return npe.value


@pytest.mark.parametrize("rows_per_item", [1, 3])
def test_four_redshifts_in_one_batch_of_thousands_of_items(eng, capfd, rows_per_item):
    prms = [plain(R5, z=z) for z in (0.01, 0.5, 1.0, 2.0)]
    new, old, (n_wg, n_items, _) = both_reported(eng, capfd, prms, T37, NU10, ppb(rows_per_item))
    assert n_items >= 2000 and n_items >= 4 * n_wg, (n_wg, n_items)  # every workgroup takes several items, of more than one model
    assert_bits(new, old)
    assert not np.array_equal(new[0], new[1]) and not np.array_equal(new[2], new[3])


# (time resolution, requested times, z) -> the lattice length K it gives; 18 K against the multiples of 512:
#   28: 504 = 512 - 8      29: 522 = 512 + 10      85: 1530 = 3 x 512 - 6      86: 1548 = 3 x 512 + 12
#   199: 3582 = 7 x 512 - 2 (the headline)      200: 3600 = 7 x 512 + 16      202: the longest the split form's LDS takes at 10 nu x 200 t
LATTICES = {28: (3.2, T37, 1.0), 29: (3.32, T37, 1.0), 85: (9.58, T37, 1.0), 86: (9.68, T37, 1.0), 182: (20.5, T37, 1.0),
            199: (20.5, configs.C2_T, 1.0), 200: (20.6, configs.C2_T, 1.0), 202: (20.5, configs.C2_T, 0.5)}


def test_the_lattice_lengths_cover_the_steps_of_the_staging():
    ks = sorted(LATTICES)
    words = [NPAR * k for k in ks]
    below = [w for w in words if 0 < -w % LANES <= NPAR]   # the next lattice length is past the multiple
    above = [w for w in words if 0 < w % LANES <= NPAR]    # the one before was short of it
    assert len(below) >= 2 and len(above) >= 2, (below, above)
    assert any(w < LANES for w in words) and any(w > 7 * LANES for w in words)  # a single pass of some lanes; an eighth word per lane
    assert any(k < 64 for k in ks) and any(64 < k < 128 for k in ks) and any(k > 128 for k in ks) and 199 in ks


@pytest.mark.parametrize("k_want", sorted(LATTICES))
def test_lattice_lengths_either_side_of_the_staging_steps(eng, capfd, k_want):
    rt, t, z = LATTICES[k_want]
    prms = [plain((0.3, 1.0, rt), z=z), plain((0.3, 1.0, rt), z=z, eps_e=0.07, p=2.6)]  # the same lattice, other spectra
    new, old, (_, _, k) = both_reported(eng, capfd, prms, t, NU10)
    assert k == k_want, (k, k_want)
    assert_bits(new, old)


def test_the_next_lattice_length_is_refused(eng, capfd):
    """K = 203 at ten frequencies and 200 times is past the split form's LDS: forced or not, the launch stays with the plain kernel."""
    prms = [plain((0.3, 1.0, 20.5), z=0.01)]
    hooks = {"VAG_DEBUG_LAUNCH": "1", "VAG_FLUX_WIDE": "1", "VAG_FLUX_PERSISTENT": "2", "VAG_FLUX_SPLIT": "2"}
    for k, v in hooks.items():
        _lib.hooks[k] = v
    try:
        capfd.readouterr()
        out, _ = grid(eng, prms, configs.C2_T, NU10)
        err = capfd.readouterr().err
    finally:
        for k in hooks:
            _lib.hooks.pop(k, None)
    assert report_of(err)[2] == 203 and "grid flux split:" not in err, err
    assert np.all(np.isfinite(out)) and out.max() > 0


@pytest.mark.parametrize("rows_per_item", [1, 2, 7])
def test_on_axis_every_row_restages_at_ten_frequencies(eng, capfd, rows_per_item):
    prms = c2(R10, 3, 141, theta_obs=0.0)
    assert n_phi_eff_of(eng, prms[0], T37) == 1
    new, old = both(eng, capfd, prms, T37, NU10, ppb(rows_per_item))
    assert_bits(new, old)


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_items_that_end_on_straddle_and_follow_the_change_of_block(eng, capfd, shift):
    """n_phi_eff - 1, n_phi_eff and n_phi_eff + 1 rows per item: over the items the re-staging falls on an item's last row, exactly
    between two items, and on an item's second row."""
    prms = [plain(R5), plain(R5, eps_B=0.02, p=2.15)]
    npe = n_phi_eff_of(eng, prms[0], T37)
    assert npe > 2 and n_phi_eff_of(eng, prms[1], T37) == npe
    new, old = both(eng, capfd, prms, T37, NU10, ppb(npe + shift))
    assert_bits(new, old)


def test_rejected_model_among_items_of_one_row(eng, capfd):
    """The batch of test_mixed_batch_with_a_rejected_model (tests/test_flux_split.py) at one row per item: claims are made across the
    model whose items return at once."""
    prms = []
    for i, res in enumerate([R10, (0.15, 0.5, 10.0), R20, (0.2, 2.0, 5.0)] * 3):
        prms += c2(res, 1, 60 + i)
    bad = _abi.make_params(**dict(configs.C2, resolutions=(200.0, 0.31, 5.0)))
    prms.insert(5, bad)
    cap = {rc for rc in range(-64, 65) if rc != 0}
    new, rc_new, _ = run_form(eng, capfd, 2, prms, T37, NU10, ppb(1), ok_rc=cap)
    old, rc_old, _ = run_form(eng, capfd, 0, prms, T37, NU10, ppb(1), ok_rc=cap)
    assert rc_new == rc_old and rc_new != 0
    good = [i for i in range(len(prms)) if i != 5]
    assert_bits(new[good], old[good])


def test_fewer_items_than_workgroups_twice_with_another_shape_between(eng, capfd):
    prms = c2(M12, 1, 171)
    a, _, err = run_form(eng, capfd, 2, prms, T37, NU10, ppb(128))  # (run_form makes a call of another shape ahead of each)
    n_wg, n_items, _ = report_of(err)
    assert n_items == n_wg and n_items < 128, (n_wg, n_items)  # a workgroup per item: fewer items than the chip holds workgroups
    b = run_form(eng, capfd, 2, prms, T37, NU10, ppb(128))[0]
    old = run_form(eng, capfd, 0, prms, T37, NU10, ppb(128))[0]
    assert_bits(a, b)
    assert_bits(a, old)
