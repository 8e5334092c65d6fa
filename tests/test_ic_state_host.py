"""The inverse-Compton reference (tests/_icref.py) on the CPU, before tests/test_ic_state.py holds the device to it:

a. attainability: a float64 restatement of every routine, in the device's statement order, against the reference on the probe sets.  The
   maximum per quantity and class is the figure beside each ceiling (_icref.CPU_FIGURES; ceiling = 25 x figure): the test measures it
   again and fails where it has grown past twice the recorded one;
b. the reference itself: the Klein-Nishina ratio at 50 digits against 100 digits and against its series at small x, the long-double
   closed forms against mpmath on a subset of rows; what linear interpolation on the 128 nodes costs is printed and not gated;
c. reach: the probe sets hold the regimes and edges they are there for, with counts;
d. sensitivity: planted defects of the restatements each land above 100 x the ceiling of the quantity they move, or break an output that
   must be exact;
e. the fixed points' bookkeeping: the admissible-iterate rule applied to the float64 restatement of the loops misses nothing, no row
   reaches a guard, and at most 2 % of the rows admit more than one stopping iterate."""
import numpy as np
import pytest

import _icref as R

np.seterr(all="ignore")
TAG = "[ic state host]"
NAMES = list(R._MAKERS)


# ---------------------------------------------------------------- a. attainability
@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_gives_the_recorded_figures(name):
    worst, counts = R.errors(name, R.f64_out(name))
    bad = []
    for key, err in sorted(worst.items()):
        fig = R.CPU_FIGURES[key]
        print(f"{TAG} {name:15s} {' '.join(key):32s} float64 {err:.2e}  recorded {fig:.1e}  ceiling {R.ceiling(*key):.1e}")
        if not err <= 2 * fig:
            bad.append(f"{key}: float64 gives {err:.3e}, recorded {fig:.1e}")
    assert not bad, "\n".join(bad)
    assert not any(counts.values()), counts
    assert set(k for k in R.CPU_FIGURES if k[0].split(".")[0] in R.PREFIX[name]) <= set(worst), "a recorded class that the probe set does not reach"


def test_every_recorded_figure_belongs_to_a_probe_routine():
    owned = {p for v in R.PREFIX.values() for p in v}
    assert {k[0].split(".")[0] for k in R.CPU_FIGURES} == owned and set(R.PREFIX) == set(NAMES)


# ---------------------------------------------------------------- b. the reference itself
def test_klein_nishina_reference_does_not_cancel_and_meets_its_series():
    mp = R.mpmath
    worst = 0.0
    for k in range(R.KN_LUT_N):
        with mp.workdps(R.KN_DPS):
            x = mp.power(2, mp.mpf(float(R.kn_node_lg2x(k))))
            a = R.kn_ratio_mp(x, 0)
        with mp.workdps(2 * R.KN_DPS):
            b = R.kn_ratio_mp(mp.power(2, mp.mpf(float(R.kn_node_lg2x(k)))), 0)
            worst = max(worst, float(abs(a - b) / b))
    print(f"{TAG} Klein-Nishina ratio at {R.KN_DPS} digits against {2 * R.KN_DPS}, on the 128 nodes: {worst:.1e}")
    assert worst <= 1e-40
    with mp.workdps(R.KN_DPS):  # sigma / sigma_T = 1 - 2x + 26/5 x^2 - 133/10 x^3 + 1144/35 x^4 - ... (the expansion of the formula)
        for x in (1e-3, 0.0134):
            x = mp.mpf(x)
            series = 1 - 2 * x + mp.mpf(26) / 5 * x ** 2 - mp.mpf(133) / 10 * x ** 3 + mp.mpf(1144) / 35 * x ** 4
            assert abs(R.kn_ratio_mp(x, 0) - series) <= 100 * x ** 5
    # the float64 host loop's nodes against the exact ratio: the worst is where the formula cancels most
    got = R.f64_kn_lut(np.arange(R.KN_LUT_N))[:, 0]
    e = R.nearest(got, [r[0] for r in R.ref_kn_lut_all()])
    k = int(np.argmax(e))
    print(f"{TAG} host loop's nodes against the exact ratio: {e.max():.2e} at node {k}, x = {2 ** R.kn_node_lg2x(k):.4f}")
    assert k == 4 and e.max() <= 2.5e-12


def test_interpolation_cost_is_printed_not_gated():
    """What the table's design costs: linear interpolation on the exact nodes against the exact function at the intervals' midpoints, and
    the jump between 1 - 2x and the Klein-Nishina formula at x = 1e-2."""
    mp = R.mpmath
    nodes = R.kn_nodes()
    lg = 0.5 * (R.kn_node_lg2x(np.arange(127)) + R.kn_node_lg2x(np.arange(1, 128)))
    c = R._interp(R.LDT, R.ld(lg), nodes)[0]
    with mp.workdps(R.KN_DPS):
        exact = np.array([R._to_ld(R.kn_ratio_mp(mp.power(2, mp.mpf(float(v))), 0)) for v in lg])
        jump = float(abs(R.kn_ratio_mp(mp.mpf(1e-2), 0) - R.kn_ratio_mp(mp.mpf(1e-2), -1)))
    print(f"{TAG} linear interpolation against the exact ratio at the midpoints: {R.rel(c.astype(np.float64), exact).max():.1e} (not gated); "
          f"jump at x = 1e-2: {jump:.1e} (not gated)")


def test_long_double_closed_forms_agree_with_mpmath():
    mp = R.mpmath
    rows = R.probe_set("ic_column_den")[0]
    pick = np.r_[np.arange(0, rows.shape[0], 67), np.arange(rows.shape[0] - 60, rows.shape[0])]
    ref = R.ref_column(rows[pick])
    want = np.array([R.column_den_mp(r) for r in rows[pick]], dtype=R.LDT)
    e = np.abs(ref - want) / np.where(want == 0, 1, np.abs(want))
    print(f"{TAG} electron_column_den, long double against mpmath on {pick.size} rows: {float(e.max()):.1e}")
    assert float(e.max()) <= 2e-17
    rows = R.probe_set("ic_bin_integral")[0]
    cls = R.bin_class(rows)
    pick = np.flatnonzero(~np.isin(cls, ("trap", "s1~1e-3")))[::41]
    ref = R.ref_bin(rows[pick])[0]
    worst = 0.0
    with mp.workdps(R.KN_DPS):
        for r, v in zip(rows[pick], ref):
            f_lo, f_hi, nu_lo, nu_hi, l_lo, l_hi, lg2r, inv, trap = (mp.mpf(float(t)) for t in r)
            s1 = 1 + (l_hi - l_lo) * inv
            want = (f_hi * nu_hi - f_lo * nu_lo) / s1 if abs(s1) > mp.mpf(1e-3) else f_lo * nu_lo * lg2r * mp.log(2)
            worst = max(worst, float(abs(R._mp(v) - want) / abs(want)))
    print(f"{TAG} power_law_bin_integral, long double against mpmath on {pick.size} rows: {worst:.1e}")
    assert worst <= 1e-15  # (the numerator cancels up to 4e3-fold at |s1| = 1e-3: 4e3 x 2^-64 in long double)


def _against_mp(ld_value, exact, scale=None):
    """|long double - mpmath| over |mpmath| (over `scale` where given); an infinity or an integer: the same one, exactly."""
    mp = R.mpmath
    if not mp.isfinite(exact):
        return 0.0 if float(ld_value) == float(exact) else np.inf
    d = abs(R._mp(ld_value) - exact)
    return float(d / scale) if scale is not None else (float(d / abs(exact)) if exact != 0 else (0.0 if d == 0 else np.inf))


def _subset(name):
    rows = R.probe_set(name)[0]
    return rows[np.r_[np.arange(0, 4096, 37), np.arange(4096, rows.shape[0], 3)]]  # every 37th random row, every third constructed one


# long double carries 5.4e-20; a value 2^e or a^b with |e|, |b ln a| up to a few hundred carries that many roundings
LD_BOUND = 2e-17


def test_long_double_icy_one_pass_gamma_a_and_tails_agree_with_mpmath():
    """The long-double restatements that share code with the float64 ones (Icy, _pass, _gamma_a, the tails of _kn_pair) against the
    mpmath forms of _icref (IcyMp, step_mp, gamma_a_mp, kn_tails_mp), which are written in linear space from the formulas alone."""
    mp = R.mpmath
    with mp.workdps(R.KN_DPS):
        rows = _subset("ic_y")
        ref, y = R._icy_out(R.LDT, rows)
        worst = np.zeros(18)
        for a, r in enumerate(rows):
            m = R.icy_mp(r)
            assert (int(ref[a, 3]), int(ref[a, 4])) == (m[3], m[4]), "regime or number of segments"
            for j in set(range(18)) - {3, 4}:
                live = (j - 5) // 3 < m[4] if 5 <= j < 14 else True
                scale = None
                if j in (6, 9, 12) and live:
                    scale = max(abs(m[j]), 1)                 # lg2_lower: as point_errors holds it
                elif j in (7, 10, 13) and live:
                    scale = R._mp(y.c_scale[(j - 7) // 3][a]) or 1  # lg2_const: against what its subtractions cancel from
                worst[j] = max(worst[j], _against_mp(ref[a, j], m[j], scale))
        print(f"{TAG} IcY, long double against mpmath on {rows.shape[0]} rows: " + " ".join(f"{n} {w:.0e}" for n, w in zip(R.ICY_OUT, worst)))
        assert worst.max() <= LD_BOUND
        rows = _subset("ic_step")
        ref = R._step_out(R.LDT, rows)
        worst = np.zeros(5)
        for a, r in enumerate(rows):
            worst = np.maximum(worst, [_against_mp(ref[a, j], v) for j, v in enumerate(R.step_mp(r))])
        print(f"{TAG} one pass, long double against mpmath on {rows.shape[0]} rows (Y_T, Y, gc_new, gM, gM of a pass): {worst}")
        assert worst.max() <= LD_BOUND and np.sum(rows[:, 1] == 0) >= 10
        rows = _subset("ic_gamma_a")
        ga, Yc, leaf = R._gamma_a(R.LDT, rows)
        worst, compared = np.zeros(2), np.zeros(5, dtype=int)
        for a, r in enumerate(rows):
            g, yc, margin = R.gamma_a_mp(r)
            if margin > R.GA_NEAR:  # (a comparison nearer than that to its threshold goes both ways in ref_gamma_a)
                worst = np.maximum(worst, [_against_mp(ga[a], g), _against_mp(Yc[a], yc)])
                compared[leaf[a]] += 1
        print(f"{TAG} gamma_a, Y_c, long double against mpmath: {worst}, rows per leaf of the ladder {compared.tolist()}")
        assert worst.max() <= LD_BOUND and compared.min() >= 8
        rows = R.probe_set("kn_corr")[0]
        lx = R._kn_lg2x(rows)
        lx = lx[(R.kn_class(lx) != "table") & np.isfinite(lx)][::23]
        z = np.zeros(lx.size, dtype=int)
        c, l = R._kn_pair(R.LDT, R.ld(lx), np.exp2(R.ld(lx)), R.kn_nodes(), z, z)
        worst = np.zeros(2)
        for a, v in enumerate(lx):
            worst = np.maximum(worst, [_against_mp(c[a], R.kn_tails_mp(v)[0]), _against_mp(l[a], R.kn_tails_mp(v)[1])])
        print(f"{TAG} the look-up's tails, long double against mpmath on {lx.size} rows: {worst}")
        assert worst.max() <= LD_BOUND and np.sum(lx < 0) >= 30 and np.sum(lx > 0) >= 30


# ---------------------------------------------------------------- c. reach
def test_probe_sets_reach_what_they_are_there_for():
    for name in NAMES:
        rows, kind = R.probe_set(name)
        assert rows.shape[0] == kind.shape[0] <= 4096 + 256 and np.sum(~np.isin(kind, ("random", "anywhere"))) <= (256 + 16) * (64 if name == "ic_suffix_scan" else 1), name  # (a scan row is a wavefront of 64 points)
    rows, kind = R.probe_set("kn_lut")
    assert np.array_equal(rows[:, 0], np.arange(128))
    rows, kind = R.probe_set("kn_corr")
    lx = R._kn_lg2x(rows)
    node = R.kn_node_lg2x(np.arange(128))
    assert all(np.sum(lx == v) >= 1 for v in node) and all(np.sum(lx == v) >= 1 for v in 0.5 * (node[:-1] + node[1:]))
    for end in (R.KN_LG2_XMIN, R.KN_LG2_XMAX):
        for k in (-1, 0, 1):
            assert np.sum(rows[:, 1] == R.nudge(end, k)) >= 1, (end, k)
        assert np.sum(np.isnan(rows[:, 1]) & (np.abs(rows[:, 0] + R.LG2_X_PER_NU - end) < 1e-13)) >= 3
    assert lx[np.isfinite(lx)].min() <= R.KN_LG2_XMIN - 20 and lx.max() >= R.KN_LG2_XMAX + 20
    assert np.sum(np.isneginf(rows[:, 0])) == 2 and np.sum(np.isnan(rows[:, 1])) >= 4000
    for c in ("below", "table", "above"):
        assert np.sum(R.kn_class(lx) == c) >= 500, c
    rows, kind = R.probe_set("ic_table")
    n = rows[:, 0]
    for v in (-1, 0, 1, 2, 3, 16):
        assert np.sum(n == v) >= 20, v
        for k in ("first", "last", "last+1", "last-1", "th_min < x < first", "last < x < th_max", "x < th_min", "x > th_max"):
            assert np.sum((n == v) & (kind == k)) >= 1, (v, k)
        assert np.sum((n == v) & (kind == "node")) == max(v, 0)
    refs = R.ref_table(rows)
    live = n >= 2
    assert np.all((refs[0][1][kind == "th_min < x < first"] & 1) == live[kind == "th_min < x < first"])
    assert np.all((refs[0][1][kind == "last < x < th_max"] & 1) == live[kind == "last < x < th_max"])
    assert not np.any(refs[0][1][np.isin(kind, ("x < th_min", "x > th_max", "x = th_min", "x = th_max"))] & 1)
    assert np.all((refs[0][1][n < 0] & 4) == 4) and not np.any(refs[0][1][n >= 0] & 4)
    assert np.all(np.isneginf(refs[0][0][kind == "last+2"].astype(np.float64))) and np.all(np.isneginf(refs[1][0][kind == "last+2"].astype(np.float64)))
    assert np.all(np.isfinite(refs[0][0][(kind == "last") & live].astype(np.float64)))
    assert np.all(np.isnan(rows[:, 5:][np.arange(16)[None, :] >= np.maximum(n, 0)[:, None]])), "NaN past the table's n words"
    rows, kind = R.probe_set("ic_bin_integral")
    cls = R.bin_class(rows)
    s1 = R._bin(R.LDT, rows, None)[1].astype(np.float64)
    assert np.sum(rows[:, 0] == 0) >= 8 and np.sum(rows[:, 1] == 0) >= 8 and np.sum(cls == "trap") >= 24
    for sgn in (1, -1):
        assert np.sum((np.sign(s1) == sgn) & (cls == "s1~1e-3")) >= 60 and np.sum((np.sign(s1) == sgn) & (cls == "series")) >= 16
        assert np.sum((np.sign(s1) == sgn) & (np.abs(s1) > 100)) >= 100 and np.sum((np.sign(s1) == sgn) & (np.abs(s1) < 1e-2)) >= 100
        grid = np.array([k.startswith("s1 on the grid") for k in kind]) & (np.sign(s1) == sgn)
        assert len(np.unique(s1[grid])) == 5 and np.sum(np.abs(s1[grid]) > 1e-3) >= 8 and np.sum(np.abs(s1[grid]) <= 1e-3) >= 8
    rows, kind = R.probe_set("ic_suffix_scan")
    assert rows.shape[0] % 64 == 0 and np.all(rows >= 0)
    for k, least in (("random", 8), ("one-hot", 9), ("zero", 1), ("equal", 1)):
        assert np.sum(kind == k) == 64 * np.sum(kind == k) // 64 >= 64 * least, k
    w = rows[kind == "random"]
    assert np.log10(w.max() / w.min()) >= 29
    rows, kind = R.probe_set("ic_column_den")
    for r in range(7):
        assert np.sum(rows[:, 5] == r) >= 400, r
    for k in ("gamma < gamma_c", "gamma = gamma_c", "gamma > gamma_c"):
        assert np.sum(kind == k) >= 80, k
    assert np.all(rows[kind == "gamma = gamma_c", 0] == rows[kind == "gamma = gamma_c", 2])
    assert np.sum(np.isinf(rows[:, 3])) >= 200 and (rows[:, 0] / rows[:, 1]).max() > 5e7 and (rows[:, 0] / rows[:, 1]).min() < 1.01
    assert set(np.unique(rows[:, 4])) == {2.01, 2.3, 2.999, 3.0, 3.5}
    rows, kind = R.probe_set("ic_y")
    y = R._icy_out(np.float64, rows)[1]
    for r in (0, 1, 2):
        assert np.sum(y.regime == r) >= 900, r
    for k in ("gamma_c < gamma_m", "gamma_c = gamma_m", "gamma_c > gamma_m"):
        assert np.sum(kind == k) >= 20, k
    assert np.all(rows[kind == "gamma_c = gamma_m", 0] == rows[kind == "gamma_c = gamma_m", 1])
    for m_one in (False, True):
        for c_one in (False, True):
            assert np.sum((kind != "random") & ((y.gm_hat == 1) == m_one) & ((y.gc_hat == 1) == c_one)) >= 40, (m_one, c_one)
    kn = rows[:, 5] != 0
    for lower in (y.l[1], y.l[2]):  # g on each break and 1, 2 steps either side
        for k in (-2, -1, 0, 1, 2):
            assert np.sum(kn & (rows[:, 7] == R.nudge(np.exp2(lower), k))) >= 100, k
    assert set(np.unique(rows[:, 2])) == set(R.P_SET) and rows[:, 3].min() < 2e-6 and rows[:, 3].max() > 5e3
    assert rows[:, 4].min() < 2e-8 and rows[:, 4].max() > 5e3
    rows, kind = R.probe_set("ic_step")
    assert np.sum(rows[:, 1] == 0) >= 64 and rows[rows[:, 1] > 0, 1].min() < 2e-6 and rows[:, 1].max() > 5e3
    assert rows[:, 5].min() < 2e-3 and rows[:, 5].max() > 5e4 and np.sum(rows[:, 6] == 0) > 1000 and np.sum(rows[:, 6] == 1) > 1000
    ref = R._step_out(R.LDT, rows)
    assert np.all(np.isinf(ref[rows[:, 1] == 0, 2:].astype(np.float64))) and np.all(np.isfinite(ref[rows[:, 1] > 0].astype(np.float64)))
    for c, least in (("Y_T>=1e-3", 1000), ("Y_T<1e-3", 100), ("Y_T<1e-4", 50), ("Y_T<1e-5", 30), ("Y_T<1e-6", 20), ("Y_T<1e-7", 20), ("Y_T<1e-8", 10)):
        assert np.sum(R.yt_class(ref[:, 0]) == c) >= least, c
    rows, kind = R.probe_set("ic_gamma_a")
    leaf = R._gamma_a(np.float64, rows)[2]
    for k, name in enumerate(R.LEAVES):
        assert np.sum(leaf == k) >= 64, name
    made = kind == "ordering"
    reg = R.determine_regime(rows[:, 8], rows[:, 9], rows[:, 10])
    for r in range(1, 7):
        assert np.sum(made & (reg == r)) >= 16, r
    a, c, m = rows[kind == "tie", 8], rows[kind == "tie", 9], rows[kind == "tie", 10]
    assert np.sum((a == c) & (c == m)) >= 16 and np.all(reg[kind == "tie"] > 0)
    for pair in ((a == c) & (c != m), (a == m) & (c != m), (c == m) & (a != m)):
        assert np.sum(pair) >= 32  # (either side of the third)
    rows, kind = R.probe_set("ic_fixed_point")
    ans = R._fixed_answer(rows)
    f = rows[:, 4] / ans
    assert f.min() < 3e-3 and f.max() > 3e2 and np.sum(kind == "one pass") >= 64 and np.sum(kind == "on the threshold") >= 48
    assert np.all(rows[:, 1] > 0) and (rows[:, 8] * np.sqrt(rows[:, 1] / R.er.K_GAMMA_M)).min() < 3e-3


# ---------------------------------------------------------------- d. sensitivity
def _on_last(r):
    """Rows of the ic_table set whose (x - first) / step reaches n - 1 as a double: where x = last asks the clamp for anything (on the
    others the quotient rounds just below n - 1 and the floor is n - 2 by itself)."""
    return np.floor((r[:, 4] - r[:, 1]) * R.IC_INV_STEP) >= r[:, 0] - 1


def _ratio(name, mut, quantity, active=None):
    """Per point the defect moves: its error over 100 x the ceiling of its class."""
    pe, _ = R.point_errors(name, R.f64_out(name, (mut,)))
    err, key, idx = pe[quantity]
    ratio = err / (100 * R.key_ceilings(key))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if active is not None:
        ratio = ratio[active(R.probe_set(name)[0][idx], R.probe_set(name)[1][idx])]
    return ratio


@pytest.mark.parametrize("mut,name,quantity,active,least,every", [
    ("low_tail_first_order_log", "kn_corr", "lg2.lg2_corr", lambda r, k: R.kn_class(r[:, 0] + R.LG2_X_PER_NU) == "below", 30, False),
    ("low_tail_first_order_log", "kn_corr", "node.lg2_corr", lambda r, k: R.kn_class(R._kn_lg2x(r)) == "below", 30, False),
    ("first_order_ln2x", "kn_corr", "lg2.corr", lambda r, k: R.kn_class(r[:, 0] + R.LG2_X_PER_NU) == "above", 30, False),
    ("high_tail_without_half", "kn_corr", "node.lg2_corr", lambda r, k: R.kn_class(R._kn_lg2x(r)) == "above", 30, False),
    ("idx_not_clamped", "ic_table", "table.value", lambda r, k: (k == "last") & (r[:, 0] >= 2) & (r[:, 0] < 16) & _on_last(r), 30, True),
    ("frac_before_clamp", "ic_table", "table.value", lambda r, k: (k == "last") & (r[:, 0] >= 2) & _on_last(r), 30, True),
    ("frac_before_clamp", "ic_table", "table.value", lambda r, k: (k == "th_min < x < first") & (r[:, 0] >= 2), 5, True),
    ("rcp_without_newton", "ic_bin_integral", "bin", lambda r, k: ~np.isin(R.bin_class(r), ("series", "s1~1e-3")), 30, False),
    ("series_branch_at_any_s1", "ic_bin_integral", "bin", lambda r, k: ~np.isin(R.bin_class(r), ("series", "s1~1e-3")), 30, False),
    ("scan_drops_lane63", "ic_suffix_scan", "scan", lambda r, k: np.isin(k, ("equal", "random")), 30, False),
    ("ic_factor_below_gamma_c", "ic_column_den", "column_den", lambda r, k: r[:, 0] <= r[:, 2], 30, False),
    ("regime_sets_swapped", "ic_column_den", "column_den", None, 30, False),
    ("mid_slope_p_minus_2", "ic_y", "icy.slope", lambda r, k: (r[:, 5] != 0) & (r[:, 0] < r[:, 1]), 30, False),
    ("mid_slope_p_minus_2", "ic_step", "step.gc_new", lambda r, k: (r[:, 6] != 0) & (r[:, 2] < r[:, 3]) & (k == "random"), 30, False),
    ("segment_1_at_a_tie", "ic_y", "icy.Y", lambda r, k: k == "hats clamped clamped", 30, True),
    ("gamma_c_without_plus_4", "ic_step", "step.gc_new", lambda r, k: k == "random", 30, False),
    ("gamma_c_without_plus_4", "ic_fixed_point", "fixed.gc", lambda r, k: k == "random", 30, False),
    ("gamma_a_without_plus_1", "ic_gamma_a", "ga.gamma_a", None, 30, False),
    ("gamma_a_without_ic_factor", "ic_gamma_a", "ga.gamma_a", lambda r, k: np.isin(R._gamma_a(np.float64, r)[2], (2, 4)) & (r[:, 6] > 1) & (r[:, 7] != 0), 30, False),  # (Thomson: Y is one number, the factor 1)
])
def test_reference_sees_a_defect(mut, name, quantity, active, least, every):
    """Each defect moves the MEDIAN point it applies to by more than 100 x the ceiling of that point's class; a defect confined to
    constructed rows (`every`) moves EVERY one of them by that much."""
    assert mut in R.MUTATIONS
    ratio = _ratio(name, mut, quantity, active)
    assert ratio.size >= least, f"{mut}: only {ratio.size} points exercise it"
    print(f"{TAG} {mut:32s} {quantity:14s} error / (100 x ceiling): median {np.median(ratio):.2e}, smallest {ratio.min():.2e}, on {ratio.size} points")
    assert np.median(ratio) > 1 and (not every or ratio.min() > 1)


def test_reference_sees_wrong_breach_bits():
    mut = "breach_ignores_theoretical_range"
    assert mut in R.MUTATIONS
    _, counts = R.point_errors("ic_table", R.f64_out("ic_table", (mut,)))
    rows, kind = R.probe_set("ic_table")
    outside = np.sum(np.isin(kind, ("x < th_min", "x > th_max", "x = th_min", "x = th_max")) & (rows[:, 0] >= 2))
    print(f"{TAG} {mut}: {counts} of {outside} constructed rows outside the theoretical range")
    assert sum(counts.values()) >= outside >= 12


# ---------------------------------------------------------------- e. the fixed points' bookkeeping
def test_fixed_point_bookkeeping():
    """Conditions on the probe set, from the reference alone: no row reaches a guard (100 / 10000 passes), at most 2 % of the rows admit
    more than one stopping iterate, the rows built on the threshold do, the one-pass rows take one pass.  Then the float64 restatement of
    the loops through the admissible-iterate rule: every pass count admitted."""
    rows, kind = R.probe_set("ic_fixed_point")
    out = R.f64_out("ic_fixed_point")
    err, info = R.fixed_errors(rows, out)
    print(f"{TAG} delta = {R.stop_margin():.1e}; rows admitting more than one iterate: gamma_c {np.mean(info['count'] > 1):.2%}, gamma_M "
          f"{np.mean(info['count_M'] > 1):.2%}; most passes: gamma_c {int(out[:, 3].max())}, gamma_M {int(out[:, 5].max())}")
    assert not info["guard"].any() and not info["guard_M"].any()
    assert np.all(info["count"] >= 1) and np.all(info["count_M"] >= 1)
    assert np.mean(info["count"] > 1) <= 0.02 and np.mean(info["count_M"] > 1) <= 0.02
    assert np.mean(info["count"][kind == "on the threshold"] > 1) >= 0.8
    kn = rows[:, 7] != 0
    one = kind == "one pass"  # (without Klein-Nishina the cell's own gamma_c may already be within 1e-3: no pass at all)
    assert np.all(out[one & kn, 3] == 1) and np.all(out[one & ~kn, 3] <= 1) and np.sum(out[one, 3] == 1) >= 48
    assert out[:, 3].max() < 100 and np.sum(out[:, 3] == 0) >= 5
    assert np.mean(out[kn, 0] != out[kn, 1]) > 0.5 and np.all(out[~kn, 0] == out[~kn, 1])  # gc_used: the last pass's argument (KN) or gc itself
    assert np.all(np.isfinite(err["fixed.gc"])) and np.all(np.isfinite(err["fixed.gM"])), "a pass count of the float64 loop that the rule does not admit"


def test_every_defect_is_exercised():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_every_defect_is_exercised))
    assert all(src.count(f'"{m}"') >= 1 for m in R.MUTATIONS)
    assert len(R.MUTATIONS) >= 10
