"""The reverse-shock state reference (tests/_rsref.py) on the CPU, before tests/test_reverse_state.py holds the device to it:

a. attainability: a float64 restatement of every routine, in the device's statement order, against the reference on the probe sets.  The
   maximum per quantity and class is the figure beside each ceiling (_rsref.CPU_FIGURES; ceiling = 25 x figure): the test measures it
   again and fails where it has grown past twice the recorded one;
b. the reference of the cubic against mpmath.polyroots with the same selection rule, on a subset;
c. the fast forms: the bound on |fast - exact| from an exact reciprocal and square root, each call moved by +- the project's figures
   for rcp1 (2.2e-15) and sqrt1 (4.2e-15), every sign pattern (_rsref.FAST_BOUNDS);
d. sensitivity: ten defects of the restatements each land above 100 x the ceiling of the quantity they move;
e. the lattices: the integers against the reference exactly, ascending nodes, and that the set reaches every edge rule;
f. what the metric leaves out: the error of rel_Gamma relative to Gamma34 - 1, printed and not gated."""
import numpy as np
import pytest

import _rsref as R

np.seterr(all="ignore")
TAG = "[reverse state host]"


def f64_out(name, mut=()):
    """The float64 restatement's outputs on probe_set(name), in the probe routine's column order."""
    rows = R.probe_set(name)[0]
    if name == "rel_gamma":
        return np.stack([R.f64_rel_Gamma(rows[:, 0], rows[:, 1], mut)] * 2, axis=1)
    if name == "shock_jump":
        g, s = rows[:, 0], rows[:, 1]
        return np.stack([R.f64_downstr_4vel(g, s, mut), R.f64_jump_4vel(g, s, mut), R.f64_jump_4vel_f(g, s, mut)], axis=1)
    if name == "sound_speed":
        return np.stack([R.f64_sound_speed(rows[:, 0])] * 2, axis=1)
    if name == "rvs_state":
        return R.f64_rvs_state(rows, mut)
    if name == "rvs_extrap":
        return R.f64_extrap(rows, mut)[0].reshape(rows.shape[0], -1)
    if name == "pair_init":
        return R.f64_init(rows)
    raise KeyError(name)


# ---------------------------------------------------------------- a. attainability
@pytest.mark.parametrize("name", ["rel_gamma", "shock_jump", "sound_speed", "rvs_state", "rvs_extrap", "pair_init"])
def test_float64_restatement_gives_the_recorded_figures(name):
    worst, counts = R.errors(name, f64_out(name))
    bad = []
    for key, err in sorted(worst.items()):
        if key in R.FAST_BOUNDS:  # (the restatement's fast columns are its exact ones: section c)
            continue
        fig = R.CPU_FIGURES[key]
        print(f"{TAG} {name:11s} {' '.join(key):40s} float64 {err:.2e}  recorded {fig:.1e}  ceiling {R.ceiling(*key):.1e}")
        if not err <= 2 * fig:
            bad.append(f"{key}: float64 gives {err:.3e}, recorded {fig:.1e}")
    assert not bad, "\n".join(bad)
    assert not any(counts.values()), counts
    assert set(k for k in R.CPU_FIGURES if k[0].split(".")[0] in {"rel_gamma": ("rel_Gamma",), "shock_jump": ("u_down", "jump"),
               "sound_speed": ("sound_speed",), "rvs_state": ("rvs",), "rvs_extrap": ("extrap",), "pair_init": ("init",)}[name]) <= set(worst), \
        "a recorded class that the probe set does not reach"


def test_probe_sets_reach_what_the_issue_names():
    rows, kind = R.probe_set("shock_jump")
    gm1, s = rows[:, 0] - 1, rows[:, 1]
    assert rows.shape[0] <= 4096 + 256 and gm1[kind == "random"].min() < 1e-14 and gm1.max() > 1e2
    for k in (-2, -1, 0, 1, 2):
        assert np.sum(s == R.nudge(R.SIGMA_CUT, k)) >= 32
    assert np.sum(s == 0) > 500 and np.sum((s > R.SIGMA_CUT) & (s <= 10 * R.SIGMA_CUT)) > 500 and s.max() > 1e2
    rows, kind = R.probe_set("rel_gamma")
    assert np.sum(rows[:, 0] == rows[:, 1]) >= 64 and np.sum(rows[:, 1] == 1) >= 64
    rows, kind = R.probe_set("rvs_extrap")
    for k in ("idx_cut == 0", "idx_cut >= nt - 2", "idx_cut >= inj", "applies"):
        assert np.sum(kind == k) >= 30, k
    rows, kind = R.probe_set("pair_init")
    st = R.f64_init(rows)
    seeded = st[:, R.STATE.index("m3")] != 0
    assert np.all(st[:, R.STATE.index("Gamma")] > 1.03), "a row the kernel would not integrate"
    for wind in (0, 1):
        m = rows[:, 6] == wind
        assert np.sum(m & (rows[:, 4] < rows[:, 3])) > 100 and np.sum(m & (rows[:, 4] > rows[:, 3])) > 100
    assert np.sum(~seeded) >= 64 and np.sum(seeded) > 500  # Gamma34 == 1 exactly: nothing seeded
    assert np.all(R.f64_rel_Gamma(rows[~seeded, 0], st[~seeded, 0]) == 1.0)
    rows, kind = R.probe_set("rvs_state")
    gc, sc = R.rvs_classes(rows)
    for g in R._G:
        for s_ in R._S:
            for flag in (0, 1):
                assert np.sum((gc == g) & (sc == s_) & (rows[:, 10] == flag)) >= 30, (g, s_, flag)


# ---------------------------------------------------------------- b. the cubic
def test_cubic_reference_agrees_with_polyroots():
    """The trigonometric solution at CUBIC_DPS digits against mpmath.polyroots on the same coefficients, with the device's selection rule."""
    mp = R.mpmath
    rows, kind = R.probe_set("shock_jump")
    mag = np.flatnonzero(rows[:, 1] > R.SIGMA_CUT)
    pick = mag[np.argsort(rows[mag, 0])][:: max(1, mag.size // 48)]  # across gamma_rel - 1 from 1e-15 up
    worst = 0.0
    with mp.workdps(R.CUBIC_DPS):
        for i in pick:
            g, s = mp.mpf(float(rows[i, 0])), mp.mpf(float(rows[i, 1]))
            b, c, d = R.cubic_coefficients(g, s)
            roots = mp.polyroots([1, b, c, d], maxsteps=200, extraprec=400)
            assert all(abs(mp.im(r)) <= mp.mpf(10) ** -60 * max(1, abs(r)) for r in roots), "a complex root: the selection rule has no meaning"
            real = sorted(mp.re(r) for r in roots)
            want = mp.sqrt(max(real[1], 0)) if real[2] > 0 else mp.mpf(0)
            got = R.cubic_u_down_mp(g, s)
            worst = max(worst, float(abs(got - want) / want))
    print(f"{TAG} cubic, trigonometric against polyroots on {pick.size} points: {worst:.1e}")
    assert worst <= 1e-30


# ---------------------------------------------------------------- c. the fast forms
def test_fast_form_bounds():
    rows = R.probe_set("rel_gamma")[0]
    g1, g2 = rows[:, 0], rows[:, 1]
    got = {("|rel_Gamma_f - rel_Gamma|",): R.fast_bound(lambda op: R.f64_rel_Gamma(g1, g2, op=op), 2, R.f64_rel_Gamma(g1, g2)).max()}
    rows = R.probe_set("shock_jump")[0]
    hyd = rows[:, 1] <= R.SIGMA_CUT
    g, s = rows[hyd, 0], rows[hyd, 1]
    b = R.fast_bound(lambda op: R.f64_jump_4vel_f(g, s, op=op), 5, R.f64_jump_4vel(g, s))
    gc = R.gclass(g - 1)
    got.update({("|jump_f - jump|", c): b[gc == c].max() for c in R._G})
    G = R.probe_set("sound_speed")[0][:, 0]
    got["|sound_speed_f - sound_speed|",] = R.fast_bound(lambda op: R.f64_sound_speed(G, op=op), 3, R.f64_sound_speed(G)).max()
    for key, v in got.items():
        print(f"{TAG} {' '.join(key):40s} bound {v:.2e}  recorded {R.FAST_BOUNDS[key]:.1e}")
        assert 0.5 * R.FAST_BOUNDS[key] <= v <= R.FAST_BOUNDS[key], (key, v)
    # unperturbed, the fast restatement is the exact one up to a rounding: the bound is all perturbation
    assert R.rel(R.f64_jump_4vel_f(g, s), R.ld(R.f64_jump_4vel(g, s))).max() <= 4 * 2.0 ** -52


# ---------------------------------------------------------------- d. sensitivity
def _ratio(name, mut, quantity, active=None):
    """Per point the defect moves: its error over 100 x the ceiling of its class."""
    pe, _ = R.point_errors(name, f64_out(name, (mut,)))
    err, key, idx = pe[quantity]
    with np.errstate(all="ignore"):
        ratio = err / (100 * R.key_ceilings(key))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)  # (a ceiling of 0: any change is past it)
    if active is not None:
        ratio = ratio[active(R.probe_set(name)[0][idx], R.probe_set(name)[1][idx])]
    return ratio


def _crossing(flag):
    return lambda r, k: (r[:, 10] == flag) & (k == "random")


@pytest.mark.parametrize("mut,name,quantity,active", [
    ("vieta_other_root", "shock_jump", "u_down", lambda r, k: r[:, 1] > R.SIGMA_CUT),
    ("sigma_lt_cut", "shock_jump", "u_down", lambda r, k: r[:, 1] == R.SIGMA_CUT),
    # (where g2 is within 1e-4 of g1, Gamma34 is 1 to a few 1e-9 with or without the term)
    ("rel_gamma_no_u1u2", "rel_gamma", "rel_Gamma", lambda r, k: (k == "random") & (r[:, 1] > 1) & (r[:, 1] < r[:, 0] * (1 - 1e-4))),
    ("ad_four_thirds", "shock_jump", "jump", lambda r, k: (r[:, 1] == 0) & (r[:, 0] < 10)),
    ("ad_four_thirds", "rvs_state", "rvs.rho3", lambda r, k: (k == "random") & (r[:, 6] == r[:, 8] * r[:, 7])),
    ("post_compression_inverted", "rvs_state", "rvs.B", _crossing(0)),
    ("limiter_after_crossing", "rvs_state", "rvs.Gamma_th", lambda r, k: (r[:, 10] == 0) & (r[:, 4] < 0.9e-6 * r[:, 3]) & (r[:, 3] > 0)),
    ("gamma_th_with_m4", "rvs_state", "rvs.Gamma_th", lambda r, k: (k == "random") & (r[:, 4] > 2e-6 * r[:, 3])),
    ("slope_from_next_node", "rvs_extrap", "extrap.B", None),
])
def test_reference_sees_a_defect(mut, name, quantity, active):
    """Each defect moves the MEDIAN point it applies to by more than 100 x the ceiling of that point's class."""
    assert mut in R.MUTATIONS
    ratio = _ratio(name, mut, quantity, active)
    assert ratio.size >= 30, f"{mut}: only {ratio.size} points exercise it"
    print(f"{TAG} {mut:26s} {quantity:12s} error / (100 x ceiling): median {np.median(ratio):.2e}, smallest {ratio.min():.2e}, on {ratio.size} points")
    assert np.median(ratio) > 1


@pytest.mark.parametrize("mut", ["n_pre_without_shared_node", "second_segment_node0_twice"])
def test_reference_sees_a_lattice_defect(mut):
    assert mut in R.MUTATIONS
    lats = [lat for lat in R.lattice_set() if not R.f64_lattice(*lat)["plain"]]
    assert len(lats) >= 30
    caught = 0
    for lat in lats:
        worst, problems = R.lattice_errors([lat], [R.f64_lattice(*lat, mut=(mut,))])
        caught += bool(problems) or worst > 100 * R.ceiling("lattice.node")
    print(f"{TAG} {mut}: caught on {caught} of {len(lats)} refined lattices")
    assert caught == len(lats)


# ---------------------------------------------------------------- e. the lattices
def test_lattices_follow_the_reference_and_the_set_reaches_every_edge_rule():
    lats = R.lattice_set()
    made = [R.f64_lattice(*lat) for lat in lats]
    worst, problems = R.lattice_errors(lats, made)
    print(f"{TAG} lattice nodes: float64 {worst:.2e}  recorded {R.CPU_FIGURES['lattice.node',]:.1e}  ceiling {R.ceiling('lattice.node'):.1e}; "
          f"{len(lats)} lattices, {sum(lat[4] for lat in lats)} nodes")
    assert not problems, "\n".join(problems)
    assert worst <= 2 * R.CPU_FIGURES["lattice.node",]
    assert sum(lat[4] for lat in lats) <= 4096 and {lat[4] for lat in lats} >= {4, 64}
    exact = [R.ref_lattice(*lat) for lat in lats]
    raw = [10 * max(lat[2], lat[3]) for lat in lats]
    assert sum(m["plain"] and r <= lat[0] for m, r, lat in zip(made, raw, lats)) >= 10, "plain because t_refine <= ts"
    assert sum(m["plain"] and r >= lat[1] for m, r, lat in zip(made, raw, lats)) >= 10, "plain because t_refine >= t_end"
    assert sum(r == lat[0] for r, lat in zip(raw, lats)) >= 5 and sum(r == lat[1] for r, lat in zip(raw, lats)) >= 5, "t_refine on ts / t_end"
    x = [lat[5] * np.log10(lat[1] / min(max(r, lat[0]), lat[1])) / np.log10(lat[1] / lat[0]) for r, lat in zip(raw, lats)]
    refined = [not m["plain"] for m in made]
    assert sum(f and v < 2 and m["n_post"] == 2 for f, v, m in zip(refined, x, made)) >= 5, "n_post clamped at 2"
    assert sum(f and v >= lat[4] and m["n_post"] == lat[4] // 2 for f, v, m, lat in zip(refined, x, made, lats)) >= 5, "n_post clamped at t_num / 2"
    assert sum(f and 2 <= v < lat[4] for f, v, lat in zip(refined, x, lats)) >= 10, "n_post from the ratio of the logarithms"
    for m, e in zip(made, exact):  # the shared node: node n_pre - 1 is t_refine, node n_pre the second segment's node 1
        if not m["plain"]:
            assert m["n_pre"] + m["n_post"] == len(m["nodes"]) + 1 and m["n_pre"] >= 2 and m["n_post"] >= 2


# ---------------------------------------------------------------- f. Gamma34 - 1
def test_rel_gamma_minus_one_has_lost_its_digits_and_that_is_stated():
    """rel_Gamma returns 1 + d^2 / denom, as compute_rel_Gamma does, and the right-hand side forms Gamma34 - 1 from that double.  The metric
    of these tests is the returned value; relative to Gamma34 - 1 the same rounding is as large as 1 once Gamma34 - 1 is below 1e-16.  That
    follows the reference and is not gated: this test pins the returned value and prints the other figure."""
    rows, kind = R.probe_set("rel_gamma")
    got = R.f64_rel_Gamma(rows[:, 0], rows[:, 1])
    ref = R.ref_rel_Gamma(rows[:, 0], rows[:, 1])
    m1 = (ref - 1).astype(np.float64)
    e_val = R.rel(got, ref)
    e_m1 = R.rel(got - 1, ref - 1)
    for lo, hi in ((0, 1e-16), (1e-16, 1e-12), (1e-12, 1e-6), (1e-6, np.inf)):
        sel = (m1 > lo) & (m1 <= hi)
        if sel.any():
            print(f"{TAG} Gamma34 - 1 in ({lo:g}, {hi:g}]: {int(sel.sum())} points, error of Gamma34 {e_val[sel].max():.1e}, of Gamma34 - 1 {e_m1[sel].max():.1e} (not gated)")
    assert e_val.max() <= R.ceiling("rel_Gamma")
    tiny = (m1 > 0) & (m1 < 1e-16)
    assert tiny.sum() >= 30 and e_m1[tiny].max() >= 0.5, "the set does not reach the regime this test is about"
