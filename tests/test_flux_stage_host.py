"""The flux-stage reference (tests/_fluxref.py) against the CPU oracle, on the oracle's own intermediates: the reference reads what
`details` returns (rounded to double, as the device's details are), lays out the lattice itself and must reproduce the oracle's
flux_density_grid, flux_density (series) and flux (band) to the oracle's own double rounding.  That is what entitles
tests/test_flux_stage.py to hold the device's flux stage to it.  The second half shows that the reference sees what it is for: a dropped
row, one shifted lattice node, the other bracket rule."""
import numpy as np
import pytest

import _abi
import _fluxref as fr
import _mathref as mr
import configs

# Maximum relative difference |reference - oracle| / oracle per form over the cases below, measured on the CPU build of the oracle
# (x86-64, gcc -O2, numpy.longdouble reference), 2026-10-17.  The off-axis Gaussian cases agree to 2e-14 ... 1e-13; the on-axis top hat
# and the spreading jet set the maxima: there the oracle's double Doppler factor Gamma - sqrt(Gamma^2 - 1) cos_v cancels to ~4e-11 in log2.
MEASURED = {"grid": 3.5e-12, "series": 3.5e-12, "band": 3.2e-12, "components": 5.2e-13}
# ... and per case (the larger of the three forms), so that a case the oracle computes cleanly is not held to the worst one's figure
MEASURED_CASE = {"c4_truth": 2.0e-14, "c2_small": 5.9e-14, "c2_coarse_phi": 9.3e-14, "gauss_spread": 1.4e-12, "tophat_onaxis": 3.5e-12}
GATE_FACTOR = 4  # the suite's convention (DEVIANCE_GATE, tests/test_counts.py)
CEILING = 1e-11  # a measured value above this would mean the reference is not a restatement of the stage
# the tightest case alone (C4's truth), which the sensitivity checks below are scaled to
MEASURED_C4 = MEASURED_CASE["c4_truth"]

SMALL = (0.2, 0.7, 12.0)
CASES = {
    "c4_truth": (configs.C4_TRUTH, configs.C4_EPOCHS, configs.C4_BANDS),
    "tophat_onaxis": (dict(configs.C1A, resolutions=SMALL), configs.C1_T[::5], configs.C1_NU),
    "c2_small": (dict(configs.C2, resolutions=SMALL), configs.C2_T[::8], configs.C2_NU[::3]),
    "c2_coarse_phi": (dict(configs.C2, resolutions=(0.1, 0.31, 8.0)), configs.C2_T[::8], configs.C2_NU),
    "gauss_spread": (dict(jet="GaussianJet", spreading=True, theta_obs=0.15, resolutions=(0.1, 0.3, 5.0)), configs.SPREAD_T,
                     configs.SPREAD_NU),
}
RS_NAME = "rs_thick_offaxis"


def stage_of(oracle, kw, t, rvs=False):
    prm = _abi.make_params(**kw)
    d = oracle.details(prm, float(np.min(t)), float(np.max(t)))
    cells = fr.cells_from_oracle(d, oracle.details(prm, float(np.min(t)), float(np.max(t)), rvs=True) if rvs else None)
    st = fr.FluxStage(cells, prm.rvs_p if rvs else prm.p, prm.z, prm.lumi_dist, prm.theta_obs, bool(kw.get("spreading")))
    return prm, d, st


def rel_err(flux, want):
    """Maximum relative difference of a reference Flux from the double result `want` over the slots where `want` is normal."""
    ref = flux.nearest(want)
    ok = want > 1e-250
    assert ok.mean() >= 0.98, "more than 2 % of the slots are below 1e-250"
    assert np.all(mr.to_float(ref[~ok]) < 1e-250)
    return float(np.max(np.abs(ref[ok] - want[ok]) / want[ok]))


def check(name, form, err):
    gate = GATE_FACTOR * min(MEASURED[form], MEASURED_CASE.get(name, 1.0))
    print(f"[flux stage host] {name:16s} {form:10s} measured {err:.2e}  gate {gate:.2e}")
    assert err <= gate, f"{name} {form}: {err:.3e} > {gate:.3e}"
    assert err < CEILING and MEASURED[form] < CEILING


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, oracle):
    kw, t, nu = CASES[request.param]
    prm, d, st = stage_of(oracle, kw, t)
    return request.param, prm, d, st, np.asarray(t), np.asarray(nu)


def test_lattice_is_the_oracles(case):
    """The lattice the reference lays out from r, Gamma, t_src and theta is the one observe() built (to the oracle's double rounding:
    the Doppler factor's cancellation, and cos(theta_hi) - cos(theta_lo) of a narrow ring)."""
    name, prm, d, st, t, nu = case
    assert st.shape == d["lg2_t"].shape
    if name == "tophat_onaxis":
        assert d["shape"]["n_phi_eff"] == 1
    for key, bound in (("lg2_t", 1e-10), ("lg2_doppler", 1e-9), ("lg2_geom", 1e-8)):
        fin = np.isfinite(d[key])
        assert fin.mean() > 0.97
        assert float(np.max(np.abs(st.lat[key][fin] - d[key][fin]))) < bound, key


def test_oracle_details_carry_the_polar_angle_per_cell(case):
    """extra[16] of vag_oracle_details (added for this reference: observe() of a spreading jet reads the EVOLVED angle of every cell,
    which no other details array holds): the grid angle on a jet that does not spread, an angle that only grows on one that does."""
    name, prm, d, st, t, nu = case
    th = d["theta_cell"]
    assert th.shape == d["t_src"].shape
    if name == "gauss_spread":
        assert np.all(np.diff(th, axis=1) >= 0) and np.mean(th[:, -1] > 1.01 * d["theta"]) > 0.5
        assert np.all(th[:, 0] >= d["theta"] * (1 - 1e-12))
    else:
        assert np.array_equal(th, np.repeat(d["theta"][:, None], th.shape[1], axis=1))


def test_grid_form(case, oracle):
    name, prm, d, st, t, nu = case
    check(name, "grid", rel_err(st.grid(t, nu), oracle.flux_density_grid(prm, t, nu)))


def test_series_form(case, oracle):
    name, prm, d, st, t, nu = case
    ts, ns = np.repeat(t, nu.size), np.tile(nu, t.size)  # ascending times, runs of unequal frequencies
    check(name, "series", rel_err(st.series(ts, ns), oracle.flux_density(prm, ts, ns)))


def test_band_form(case, oracle):
    name, prm, d, st, t, nu = case
    for num_nu in (5, 9, 8) if name == "c4_truth" else (5, 9):  # one Boole panel, two, and a panel plus a Simpson 3/8 tail
        check(name, "band", rel_err(st.band(t, 1e14, 1e16, num_nu), oracle.flux(prm, t, 1e14, 1e16, num_nu)))


def test_forward_and_reverse_shock_components(oracle):
    """A thick shell: both synchrotron components, each against its own reference (the reverse shock radiates on the forward shock's
    lattice with its own p)."""
    kw, t, nu = configs.RS_CASES[RS_NAME]
    kw = dict(kw, resolutions=SMALL)
    prm, d, fwd = stage_of(oracle, kw, t)
    _, _, rvs = stage_of(oracle, kw, t, rvs=True)
    want = oracle.flux_components4(prm, t, nu)
    assert want[0].max() > 0 and want[2].max() > 0
    check(RS_NAME + " fwd", "components", rel_err(fwd.grid(t, nu), want[0]))
    check(RS_NAME + " rvs", "components", rel_err(rvs.grid(t, nu), want[2]))


def test_boole_weights_integrate_power_laws():
    """compute_boole_weights: the weights integrate nu^a d nu over a decade to Boole's order on every tail."""
    for n in (2, 3, 4, 5, 8, 9, 13):
        nu = fr.band_nodes(1e14, 1e15, n)
        w = fr.boole_weights(nu)
        assert abs(float(np.sum(w) / (nu[-1] - nu[0])) - 1) < (0.5 if n == 2 else 0.05 if n < 5 else 2e-3)


# ---- sensitivity: what the reference is for ----
@pytest.fixture(scope="module")
def c4(oracle):
    kw, t, nu = CASES["c4_truth"]
    prm, d, st = stage_of(oracle, kw, t)
    base = st.grid(t, nu, keep_terms=True)
    share = mr.to_float(base.terms / base.value[None, None])  # [n_phi_eff][n_theta][nnu][nt]
    return st, np.asarray(t), np.asarray(nu), base, share


SEEN = 100 * GATE_FACTOR * MEASURED_C4  # what a defect must move to count as seen: 100 x the gate of the case


def test_sees_a_dropped_row(c4):
    st, t, nu, base, share = c4
    row_max = share.max(axis=(2, 3))
    order = np.argsort(row_max.ravel())
    i, j = np.unravel_index(order[order.size // 2], row_max.shape)  # the row of median weight
    l, s = np.unravel_index(np.argmax(share[i, j]), share[i, j].shape)
    assert share[i, j, l, s] >= 1e-6, "premise: the median row holds at least 1e-6 of the flux at its best slot"
    st.skip_rows = ((i, j),)
    try:
        got = st.grid(t, nu)
    finally:
        st.skip_rows = ()
    moved = abs(float(got.value[l, s] / base.value[l, s]) - 1)
    print(f"[flux stage host] dropped row ({i}, {j}): share {share[i, j, l, s]:.2e}, moved {moved:.2e}, must exceed {SEEN:.1e}")
    assert moved > SEEN


def test_sees_one_shifted_lattice_node(c4):
    st, t, nu, base, share = c4
    i, j, l, s = np.unravel_index(np.argmax(share), share.shape)  # the heaviest (row, slot)
    lg2_t = st.lat["lg2_t"][i, j]
    T = np.log2(np.longdouble(t[s] * mr.U_SEC))
    k = int(np.searchsorted(lg2_t, T, side="right")) - 1
    w_hi = float((T - lg2_t[k]) / (lg2_t[k + 1] - lg2_t[k]))
    node, w = (k + 1, w_hi) if w_hi >= 0.5 else (k, 1 - w_hi)  # the nearer end of the slot's bracket
    assert share[i, j, l, s] * w >= 0.02, "premise: the node carries at least 2 % of the slot"
    st.geom_shift = ((i, j, node), 1e-9)
    try:
        got = st.grid(t, nu)
    finally:
        st.geom_shift = None
    moved = abs(float(got.value[l, s] / base.value[l, s]) - 1)
    print(f"[flux stage host] node ({i}, {j}, {node}) + 1e-9: share {share[i, j, l, s]:.2e} x weight {w:.2f}, moved {moved:.2e}, "
          f"must exceed {SEEN:.1e}")
    assert moved > SEEN
    assert moved < 1e-9  # (and no more than the shift itself: ln 2 x 1e-9 x the node's share)


def test_sees_the_other_bracket_rule(c4):
    """iterate_through keeps a time on a row's last node, iterate_to drops it.  No double request lands exactly on a node of the
    extended-precision lattice, so the series is placed there in log2 (lg2_t=)."""
    st, t, nu, base, share = c4
    i, j = np.unravel_index(np.argmax(share.max(axis=(2, 3))), share.shape[:2])
    T = st.lat["lg2_t"][i, j, -1:]  # the heaviest row's last node
    through = st.series(t[-1:], nu[:1], keep_terms=True, lg2_t=T)
    to = st.series(t[-1:], nu[:1], through=False, lg2_t=T)
    held = float(through.terms[i, j, 0] / through.value[0])
    assert held >= 1e-6, "premise: the row holds at least 1e-6 of the flux at its last node"
    moved = abs(float(to.value[0] / through.value[0]) - 1)
    print(f"[flux stage host] last node of row ({i}, {j}): share {held:.2e}, moved {moved:.2e}, must exceed {SEEN:.1e}")
    assert moved > SEEN
    assert abs(moved - held) < 1e-12  # exactly that row's term
    assert 0 in through.alt and 0 in to.alt  # and both report the slot as an edge decision
