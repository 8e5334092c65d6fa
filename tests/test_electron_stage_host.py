"""The electron-stage reference (tests/_elecref.py) on the CPU, before tests/test_electron_stage.py holds the device to it:

a. attainability: a float64 restatement of the chain (pow as exp2(b log2 a), as fast_pow) agrees with the reference on the probe's own
   input set within the ceilings, link by link, with the reference's branch on every point that was not placed on a threshold -- so the
   reference alone meets the ceilings and the coverage condition;
b. sensitivity: six defects of the restatement each move their quantity by more than 100 x its ceiling (hence 100 x any gate);
c. the product path: links 1-3 on what the CPU oracle's details return for the five models of tests/test_flux_stage.py, forward shock
   and the thick shell's reverse shock, with the relic cells found from the arrays and checked against the oracle's injection index;
d. unshocked cells: the restatement gives what `_elecref.unshocked_cell` states, by class and position."""
import numpy as np
import pytest

import _abi
import _elecref as E
import _mathref as mr
import configs

np.seterr(all="ignore")

# the models of tests/test_flux_stage.py (that module needs the device library to import)
SMALL = (0.2, 0.7, 12.0)
MODELS = {
    "tophat_onaxis": dict(configs.C1A, resolutions=SMALL),
    "gauss_offaxis": dict(configs.C4_TRUTH),
    "powerlaw_wind": dict(configs.EXTRA["powerlaw_wind"][0], resolutions=(0.06, 0.2, 5.0)),
    "gauss_spread": dict(jet="GaussianJet", spreading=True, theta_obs=0.15, resolutions=(0.1, 0.3, 5.0)),
    "rs_thick": dict(configs.RS_CASES["rs_thick_offaxis"][0], resolutions=(0.06, 0.3, 8.0)),
}
T_LO, T_HI = 1e2, 1e7


def out_dict(out):
    return {n: out[:, i] for i, n in enumerate(E.OUT_NAMES)}


def probe_errors(rows, kind, out):
    """chain_errors of probe rows (the unshocked row left out) -> (errors, mask of the rows compared)."""
    sh = kind != "unshocked"
    r = rows[sh]
    e = E.chain_errors(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7], out_dict(out[sh]), r[:, 8] != 0,
                       (r[:, 9], r[:, 10], r[:, 11]))
    return e, sh


# ---------------------------------------------------------------- a. attainability
@pytest.mark.parametrize("p", E.PS)
def test_float64_restatement_meets_the_ceilings_and_the_reference_covers_every_branch(p):
    rows, kind = E.probe_set(p)
    out, nu_a2, branch = E.f64_cell(rows)
    e, sh = probe_errors(rows, kind, out)
    k, l2 = kind[sh], e["link2"]
    assert np.all(np.isfinite(out[sh])), "a shocked probe row gives a non-finite output"
    for (link, name, cls), worst in sorted(E.worst_by_class(e, rows[sh, 6]).items()):
        print(f"[electron stage host] p = {p}  link {link} {name:10s} {cls:8s} float64 {worst:.2e}  ceiling {E.ceiling(link, name, cls):.0e}")
        assert worst <= E.ceiling(link, name, cls), (link, name, cls, worst)
    # nu_a of link 2 itself, which only the restatement exposes
    err_nu, _ = l2.nearest(l2.nu_a_forms, nu_a2[sh])
    print(f"[electron stage host] p = {p}  link 2 nu_a: float64 {err_nu.max():.2e}")
    assert err_nu.max() <= E.ceiling(2, "nu_a", E.pclass(p))
    assert np.all(e["p2_ok"]), "the float64 bisection ends outside its own stop rule"
    # branches: the reference's, except on the points placed on a threshold
    free = k != "placed"
    assert np.array_equal(branch[sh][free], l2.branch[free])
    assert np.all(np.take_along_axis(l2.admissible, branch[sh][None], axis=0)[0]), "a float64 branch the reference does not admit"
    # the coverage condition, from the reference alone
    drawn = np.isin(k, ("random", "relic", "steered"))
    counts = np.bincount(l2.branch[drawn], minlength=5)
    relic = rows[sh, 8] != 0
    print(f"[electron stage host] p = {p}  branches {counts.tolist()}  slow {int((l2.slow & drawn).sum())} fast {int((~l2.slow & drawn).sum())} "
          f"relic {int((relic & drawn).sum())}  decided both ways: drawn {int(l2.both_ways[drawn].sum())}, placed "
          f"{int(l2.both_ways[k == 'placed'].sum())} of {int((k == 'placed').sum())}")
    assert counts.min() >= 100 and (l2.slow & drawn).sum() >= 100 and (~l2.slow & drawn).sum() >= 100
    assert (relic & drawn).sum() >= 100 and (~relic & drawn).sum() >= 100
    assert l2.both_ways[drawn].mean() <= 0.01
    assert l2.both_ways[k == "placed"].mean() >= 0.5, "the placed points do not sit on their thresholds"


def test_float64_shock_state_meets_its_ceiling():
    rows = E.fwd_state_rows()
    out = E.f64_fwd_state(rows)
    sh = rows[:, 3] != 0
    assert out[~sh].tolist() == [[1.0, 0.0, 0.0, 0.0]]
    r, o = rows[sh], out[sh]
    Gth, Np = E.link0_state(r[:, 2], r[:, 3])
    errs = dict(compression=E.rel(o[:, 3], E.compression(r[:, 0])), Gamma_th=E.rel(o[:, 0], Gth), N_p=E.rel(o[:, 2], Np),
                B=E.rel(o[:, 1], E.link0_B(o[:, 0], o[:, 3], r[:, 1], r[:, 4])))
    assert np.all(o[r[:, 0] <= 1, 3] == 4.0)  # no relative motion: the strong-shock limit 4 g with g = 1
    for name, v in errs.items():
        print(f"[electron stage host] link 0 {name:12s} float64 {v.max():.2e}  ceiling {E.ceiling(0, name, None):.0e}")
        assert v.max() <= E.ceiling(0, name, None) and v.max() * 25 <= 2 * E.ceiling(0, name, None)


@pytest.mark.skipif(mr.mpmath is None or not mr.LD_OK, reason="needs both backends")
def test_longdouble_reference_agrees_with_mpmath_at_40_digits():
    """The reference's own error: the longdouble chain against the same chain in mpmath at 40 digits, on points of every kind.  It must be
    far below the smallest gate (4 x 1.1e-16): 1e-17, which longdouble's eps of 1.1e-19 leaves room for through pows of exponents ~100."""
    worst = 0.0
    for p in E.PS:
        rows, kind = E.probe_set(p)
        idx = np.concatenate([np.flatnonzero(kind == k)[:6] for k in ("random", "relic", "placed", "steered", "p-ulp")])
        r = rows[idx]
        out = out_dict(E.f64_cell(r)[0])
        args = [r[:, i] for i in range(8)] + [out, r[:, 8] != 0, (r[:, 9], r[:, 10], r[:, 11])]
        a = E.chain_errors(*args, B=mr.LD)
        with mr.mpmath.workdps(40):
            b = E.chain_errors(*args, B=mr.MP)
        for key in a:
            if isinstance(key, tuple):
                assert np.array_equal(np.isnan(a[key]), np.isnan(b[key]))
                worst = max(worst, float(np.nanmax(np.abs(a[key] - b[key]))))
        assert np.array_equal(a["link2"].branch, b["link2"].branch) and np.array_equal(a["link2"].admissible, b["link2"].admissible)
        assert np.array_equal(a["p2_ok"], b["p2_ok"])
    print(f"[electron stage host] longdouble against mpmath (40 digits): {worst:.2e}")
    assert worst <= 1e-17


# ---------------------------------------------------------------- b. sensitivity
def _moved(p, mut, link, name, active):
    rows, kind = E.probe_set(p)
    out, _, _ = E.f64_cell(rows, mut=(mut,))
    e, sh = probe_errors(rows, kind, out)
    m = active(rows[sh], e["link2"]) & np.isin(kind[sh], ("random", "relic", "steered"))
    assert m.sum() >= 50, f"{mut}: only {m.sum()} points exercise it"
    v = e[link, name][m]
    v = np.where(np.isnan(v), np.inf, v)  # (a NaN where the reference has a value is as far off as can be)
    need = 100 * E.ceiling(link, name, E.pclass(p))
    print(f"[electron stage host] {mut:26s} p = {p}: {name} moved {np.median(v):.2e} (median) {v.max():.2e} (max) on {m.sum()} points, "
          f"must exceed {need:.1e}")
    return np.median(v), need


@pytest.mark.parametrize("mut,p,link,name,active", [
    ("p4_in_fast_double_break", 2.3, 2, "gamma_a", lambda r, l2: l2.branch == 4),
    ("gamma_a_without_plus_1", 2.3, 2, "gamma_a", lambda r, l2: np.ones(r.shape[0], dtype=bool)),
    ("peak_is_gamma_m", 2.3, 2, "gamma_a", lambda r, l2: ~l2.slow),
    ("f_syn_not_raised", 3.4, 2, "N_e", lambda r, l2: np.ones(r.shape[0], dtype=bool)),
    ("p_below_2_form", 2.3, 1, "gamma_m", lambda r, l2: np.ones(r.shape[0], dtype=bool)),
    ("relic_gamma_M_uncooled", 2.3, 1, "gamma_M", lambda r, l2: r[:, 8] != 0),
])
def test_reference_sees_a_defect(mut, p, link, name, active):
    """Each defect moves the MEDIAN point it applies to by more than 100 x the quantity's ceiling (and so 100 x any gate under it)."""
    assert mut in E.MUTATIONS
    moved, need = _moved(p, mut, link, name, active)
    assert moved > need


# ---------------------------------------------------------------- c. the product path on the CPU
def oracle_cells(oracle, name, rvs):
    prm = _abi.make_params(**MODELS[name])
    d = oracle.details(prm, T_LO, T_HI, rvs=rvs)
    rad = dict(p=prm.rvs_p, eps_e=prm.rvs_eps_e, xi_e=prm.rvs_xi_e) if rvs else dict(p=prm.p, eps_e=prm.eps_e, xi_e=prm.xi_e)
    cells = dict(t_comv=d["t_comv"] * mr.U_SEC, r=d["r"] * mr.U_CM, Gamma_th=d["Gamma_th"], B=d["B"] * E.U_GAUSS, N_p=d["N_p"])
    out = {n: d[n] for n in E.OUT_NAMES}  # the oracle's electron and photon arrays are in code units already
    return cells, out, rad, d["injection_idx"][:, 0].astype(int)


@pytest.mark.parametrize("name,rvs", [(n, False) for n in sorted(MODELS)] + [("rs_thick", True)])
def test_oracle_details_follow_the_chain(oracle, name, rvs):
    cells, out, rad, k_inj_oracle = oracle_cells(oracle, name, rvs)
    res = E.details_errors(cells, out, rad, rvs)
    print(f"[electron stage host] {name}{'/rvs' if rvs else ''}: {res['n']} cells, {res['n_unshocked']} unshocked, {res['n_relic']} relic, "
          f"{res['n_degenerate']} with gamma_peak = 1")
    for (link, q, cls), worst in sorted(res["worst"].items()):
        print(f"[electron stage host]   link {link} {q:10s} {cls:8s} {worst:.2e}  ceiling {E.ceiling(link, q, cls):.0e}")
        assert worst <= E.ceiling(link, q, cls), (link, q, worst)
    assert res["n"] - res["n_unshocked"] - res["n_degenerate"] > 0.5 * res["n"]
    if rvs:
        print(f"[electron stage host]   injection index: found {res['k_inj'].tolist()}  oracle {k_inj_oracle.tolist()}")
        assert np.array_equal(res["k_inj"], np.minimum(k_inj_oracle, out["gamma_m"].shape[1]))
        assert res["n_relic"] > 0 and np.all(res["k_inj"] >= 1)
    else:
        assert res["n_relic"] == 0


# ---------------------------------------------------------------- d. unshocked cells
@pytest.mark.parametrize("p", E.PS + (float(E.nudge(2.0, -1)), float(E.nudge(2.0, 1))))
def test_unshocked_cell_is_what_the_reference_states(p):
    row = E.UNSHOCKED_ROW.copy()
    row[6] = p
    rows = np.stack([row, row * np.array([7.0, 3e5, 1, 1, 1, 0.1, 1, 0.1, 1, 1, 1, 1])])  # whatever t_comv, r, eps_e, xi_e are
    out, _, _ = E.f64_cell(rows)
    want = E.unshocked_cell(p)
    print(f"[electron stage host] unshocked, p = {p!r}: " + ", ".join(f"{n} {v}" for n, v in zip(E.OUT_NAMES, want)))
    assert E.same_class(out[0], want) and E.same_class(out[1], want), out
