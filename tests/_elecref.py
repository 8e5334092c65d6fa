"""Extended-precision reference of the synchrotron electron stage alone (tests/test_electron_stage_host.py, tests/test_electron_stage.py):
what turns the shocked state of a cell (t_comv, Gamma_th, B, N_p, r) into gamma_M, gamma_m, gamma_c, N_e, the column density, I_peak,
nu_a and gamma_a, and those into the break frequencies.  Device: vag_device.h fwd_shock_state / compression_fwd, syn_elec_basic,
cool_after_crossing, the first half of syn_cell; reference sources: oracle/vag_oracle.c compute_syn_gamma_M / _gamma_m / compute_gamma_c /
cyclotron_correction / compute_syn_gamma_a / cool_after_crossing / syn_electrons_cell (synchrotron.cpp:45-110,190-246,315-360) and
save_fwd_shock_state (forward-shock.tpp:151-173).

A chain of links in numpy.longdouble (mpmath through _mathref's backends where longdouble is no wider than a double), one function each.
A link states the formula of the source it cites -- pow as 2^(b log2 a) in the backend's precision -- and takes DOUBLES as its inputs: the
test hands every link the producer's own returned doubles of the link before.  This is how the reference sources work (they store
gamma_m, gamma_c as doubles and then form (gamma_m - 1) / gamma_m and kT ~ gamma_peak - 1), and it is what makes every link well
conditioned: gamma - 1 of a stored double is exact, while a run of the whole stage from (Gamma_th, B, t_comv) differs from ANY correct
double implementation by eps / (gamma - 1).

    link 0  (Gamma, rho, U, m2, eps_B)                 -> compression ratio, Gamma_th, N_p; (Gamma_th, compression, rho, eps_B) -> B
    link 1  (t_comv, Gamma_th, B, eps_e, p, xi_e)      -> gamma_M, gamma_m, gamma_c;  relic: (inj electrons, gamma_m) -> gamma_c, gamma_M
    link 2  (gamma_m, gamma_c, B, N_p, r, p, xi_e)     -> f_syn, N_e, column density, I_peak, nu_a (branch 0 ... 4), gamma_a
    link 3  (gamma_m, gamma_c, gamma_a, gamma_M, column density, B) -> nu_m, nu_c, nu_a, nu_M, I_nu_max   (_mathref.breaks_from_physical)

Thresholds follow _mathref's `side` convention: gamma_c > gamma_m and the two nested nu_a comparisons are decided exactly and, within
THRESH_TOL of the threshold, both ways; `Link2.admissible` marks every branch some decision reaches and `Link2.nearest` compares a
produced value with the nearest admissible one.

p == 2 is a bisection stopped at a relative bracket of 1e-6 (root_bisect, utilities.h:230-241): its result is not the root to more than
that, so link 1 gives no gamma_m there; `p2_bracket_holds` states the algorithm's own stop rule instead.

Cells with B == 0 (unshocked: Gamma_th = 1, B = 0, N_p = 0) produce inf and NaN by design; the links take shocked cells only and
`unshocked_cell` states what the eleven outputs are, by class.

Everything is in the engine's code units (_mathref's U_* constants).  Under the mpmath backend the caller sets the working precision
(mpmath.workdps(40), as tests/test_mathref_host.py does)."""
import itertools

import numpy as np

import _mathref as mr

DEFAULT = mr.DEFAULT
# ---- unit constants as vag_device.h forms them (same expression order => the same doubles) ----
C_MP = mr.C_MP
C_ME = mr.C_ME
C_SIGMAT = 6.65e-25 * mr.U_CM * mr.U_CM
U_GAUSS = 8.66e-11 / mr.U_SEC
U_HZ = 1 / mr.U_SEC
U_ERG = mr.U_G * mr.U_CM * mr.U_CM / mr.U_SEC / mr.U_SEC
U_FLUX_DEN_CGS = U_ERG / (mr.U_CM * mr.U_CM) / mr.U_SEC / U_HZ

OUT_NAMES = ("gamma_m", "gamma_c", "gamma_a", "gamma_M", "N_e", "column_den", "nu_m", "nu_c", "nu_a", "nu_M", "I_nu_max")
P2_STOP = 1e-6  # root_bisect's relative bracket


def pclass(p):
    """The p class a gate belongs to: which forms of gamma_m and f_syn the cell takes."""
    return "p<2" if p < 2 else "p=2" if p == 2 else "2<p<=3" if p <= 3 else "p>3"


def _k(B, num, den=()):
    """A compound constant formed in the backend from the primitive doubles."""
    v = B.const(1.0)
    for f in num:
        v = v * B.const(f)
    for f in den:
        v = v / B.const(f)
    return v


def _pow(B, a, b):
    return B.exp2(b * B.log2(a))


def _ln(B, a):
    return B.log2(a) / B.log2e()


def rel(got, ref):
    """|got - ref| / |ref| as float64 (got: doubles, ref: backend values)."""
    ref = mr.to_ld(ref)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - ref) / np.abs(ref)).astype(np.float64)


# ---- link 0: the forward shock's state (save_fwd_shock_state; compute_compression(1, Gamma, 0), shock-physics.h:58-66,190-203) ----
def compression(Gamma, B=DEFAULT):
    G = mr._in(B, Gamma)
    one = B.const(1.0)
    g = mr._where(G > 1, one + (one - G) * (one - G) / mr._where(G > 1, G - one, one + 0 * G), one + 0 * G)  # the relative Lorentz factor
    ad = B.const(4.0) / 3 + 1 / (3 * g)
    gm1 = g - 1
    u_down = B.sqrt(np.maximum(gm1 * (ad - 1) * (ad - 1) / (-ad * (ad - 2) * gm1 + 2), 0 * g))
    u_up = B.sqrt((1 + u_down * u_down) * np.maximum((g - 1) * (g + 1), 0 * g)) + u_down * g
    zero = np.asarray(u_down == 0, dtype=bool)
    return mr._where(zero, 4 * g, u_up / mr._where(zero, one + 0 * g, u_down))


def link0_state(U, m2, B=DEFAULT):
    """Gamma_th = U / (m2 c^2) + 1 and N_p = m2 / m_p of a shocked cell (m2 != 0)."""
    U, m2 = mr._in(B, U), mr._in(B, m2)
    return U / (m2 * B.const(mr.C_C2)) + 1, m2 / B.const(C_MP)


def link0_B(Gamma_th, comp, rho, eps_B, B=DEFAULT):
    """B = sqrt(8 pi eps_B e_th), e_th = (Gamma_th - 1) rho compression c^2, from the stored doubles Gamma_th and compression."""
    Gth, comp, rho, eps_B = (mr._in(B, v) for v in (Gamma_th, comp, rho, eps_B))
    e_th = (Gth - 1) * (rho * comp) * B.const(mr.C_C2)
    return B.sqrt(8 * B.const(mr.C_PI) * eps_B * e_th)


# ---- link 1: gamma_M, gamma_m, gamma_c ----
def gamma_M_of(Bf, B=DEFAULT):
    return B.sqrt(_k(B, (6, mr.C_PI, mr.C_E), (C_SIGMAT,)) / mr._in(B, Bf))


def gamma_ave_m1(Gamma_th, eps_e, xi_e, B=DEFAULT):
    Gth, eps_e, xi_e = (mr._in(B, v) for v in (Gamma_th, eps_e, xi_e))
    return eps_e * (Gth - 1) * _k(B, (C_MP,), (C_ME,)) / xi_e


def link1(t_comv, Gamma_th, Bf, eps_e, p, xi_e, B=DEFAULT):
    """(gamma_M, gamma_m, gamma_c) of a non-relic shocked cell.  gamma_m is NaN where p == 2 (see p2_bracket_holds)."""
    t, Bv, pv = mr._in(B, t_comv), mr._in(B, Bf), mr._in(B, p)
    pf = np.broadcast_to(np.asarray(p, dtype=np.float64), np.shape(mr.to_float(Bv)))
    gM = gamma_M_of(Bf, B)
    gave = gamma_ave_m1(Gamma_th, eps_e, xi_e, B)
    hi = (pv - 2) / (pv - 1) * gave
    lo_p = mr._where(pf < 2, pv, B.const(1.5) + 0 * pv)  # keep the unused form's arguments in its domain
    lo = _pow(B, (2 - lo_p) / (lo_p - 1) * gave * _pow(B, gM, lo_p - 2), 1 / (lo_p - 1))
    gm_m1 = mr._where(pf > 2, hi, mr._where(pf < 2, lo, B.const(np.nan) + 0 * hi))
    gbar = _k(B, (6, mr.C_PI, C_ME, mr.C_C), (C_SIGMAT,)) / (Bv * Bv * t)
    gc = (gbar + B.sqrt(gbar * gbar + 4)) / 2
    return gM, gm_m1 + 1, gc


def p2_eq(x, gamma_M, gave, B=DEFAULT):
    """The p == 2 equation for x = gamma_m - 1 (gamma_m_p2_eq): x ln gamma_M - (x + 1) ln x - (gamma_ave - 1) - ln gamma_M."""
    lM = _ln(B, gamma_M)
    return x * lM - (x + 1) * _ln(B, x) - gave - lM


def p2_bracket_holds(gamma_m, Gamma_th, Bf, eps_e, xi_e, B=DEFAULT):
    """The bisection's own stop rule: the equation changes sign between (gamma_m - 1)(1 - 1e-6) and (gamma_m - 1)(1 + 1e-6), gamma_m
    the produced double."""
    x = mr._in(B, gamma_m) - 1
    gM, gave = gamma_M_of(Bf, B), gamma_ave_m1(Gamma_th, eps_e, xi_e, B)
    a, b = p2_eq(x * (1 - B.const(P2_STOP)), gM, gave, B), p2_eq(x * (1 + B.const(P2_STOP)), gM, gave, B)
    return np.asarray(a * b <= 0, dtype=bool)


def cool_after_crossing(gamma_x, gamma_m_x, gamma_m, B=DEFAULT):
    """(gamma_x - 1) (gamma_m - 1) / (gamma_m_x - 1) + 1: the crossing cell's electron cooled adiabatically to this cell."""
    gx, gmx, gm = (mr._in(B, v) for v in (gamma_x, gamma_m_x, gamma_m))
    return (gx - 1) * ((gm - 1) / (gmx - 1)) + 1


def link1_relic(inj_gamma_M, inj_gamma_m, inj_gamma_c, gamma_m, B=DEFAULT):
    """(gamma_M, gamma_c) of a relic cell from the crossing cell's stored electrons and this cell's stored gamma_m."""
    return cool_after_crossing(inj_gamma_M, inj_gamma_m, gamma_m, B), cool_after_crossing(inj_gamma_c, inj_gamma_m, gamma_m, B)


# ---- link 2: N_e, column density, I_peak, nu_a, gamma_a ----
class Link2:
    """f_syn, N_e, column_den, I_peak [n]; nu_a_forms, gamma_a_forms [5][n] (every branch's formula on every cell); branch [n] (decided
    exactly); admissible [5][n]: the branches some decision of the comparisons within THRESH_TOL of their threshold reaches."""

    def nearest(self, forms, got):
        """Per cell the relative distance of `got` (doubles) from the nearest admissible branch's value, and that branch."""
        got = np.asarray(got, dtype=np.float64)
        err = np.stack([np.where(self.admissible[b], rel(got, forms[b]), np.inf) for b in range(5)])
        err = np.where(np.isnan(err), np.inf, err)
        return err.min(axis=0), err.argmin(axis=0)

    @property
    def both_ways(self):
        return self.admissible.sum(axis=0) > 1


def link2(gamma_m, gamma_c, Bf, N_p, r, p, xi_e, B=DEFAULT):
    gm, gc, Bv, Np, rv, pv, xi = (mr._in(B, v) for v in (gamma_m, gamma_c, Bf, N_p, r, p, xi_e))
    pf = np.broadcast_to(np.asarray(p, dtype=np.float64), np.shape(mr.to_float(gm)))
    o = Link2()
    f = (gm - 1) / gm
    o.f_syn = mr._where(pf > 3, _pow(B, f, (pv - 1) / 2), f)  # cyclotron_correction
    o.N_e = Np * xi * o.f_syn
    o.column_den = o.N_e / (rv * rv)
    o.I_peak = Bv * B.const(mr.K_SYN_P) * o.column_den / B.const(4 * mr.C_PI)
    # compute_syn_gamma_a with no IC
    kf = B.const(mr.K_SYN_FREQ)
    g_peak = np.minimum(gm, gc)
    nu_peak, nu_m, nu_c = kf * Bv * g_peak * g_peak, kf * Bv * gm * gm, kf * Bv * gc * gc
    kT = (g_peak - 1) * _k(B, (C_ME, mr.C_C2), (3,))
    x = o.I_peak * B.const(mr.C_C2) / (2 * kT)
    double_break = _pow(B, x * B.sqrt(nu_c) * _pow(B, nu_m, pv / 2), 2 / (pv + 5))
    o.nu_a_forms = [
        _pow(B, x / _pow(B, nu_peak, B.const(1.0) / 3), B.const(0.6) + 0 * pv),  # 0: nu_a below the peak
        _pow(B, x * _pow(B, nu_m, pv / 2), 2 / (pv + 4)),                        # 1: slow cooling, nu_m < nu_a <= nu_c
        double_break,                                                            # 2: slow cooling, nu_a above both breaks
        _pow(B, x * B.sqrt(nu_c), B.const(0.4) + 0 * pv),                        # 3: fast cooling, nu_c < nu_a <= nu_m
        double_break,                                                            # 4: fast cooling, nu_a above both breaks
    ]
    k_ga = _k(B, (4, mr.C_PI, C_ME, mr.C_C), (3, mr.C_E))
    o.gamma_a_forms = [B.sqrt(k_ga * (nu / Bv)) + 1 for nu in o.nu_a_forms]

    def decide(s_gc, s_1, s_2):
        above = mr._gt(o.nu_a_forms[0], nu_peak, s_1)
        slow = mr._gt(gc, gm, s_gc)
        return np.where(~above, 0, np.where(slow, np.where(mr._gt(o.nu_a_forms[1], nu_c, s_2), 2, 1),
                                            np.where(mr._gt(o.nu_a_forms[3], nu_m, s_2), 4, 3)))
    o.branch = decide(None, None, None)
    o.admissible = np.zeros((5,) + o.branch.shape, dtype=bool)
    for sides in itertools.product((-1, 1), repeat=3):
        np.put_along_axis(o.admissible, decide(*sides)[None], True, axis=0)
    np.put_along_axis(o.admissible, o.branch[None], True, axis=0)
    o.slow = np.asarray(gc > gm, dtype=bool)
    o.nu_a = np.choose(o.branch, o.nu_a_forms)
    o.gamma_a = np.choose(o.branch, o.gamma_a_forms)
    o.nu_peak, o.nu_m, o.nu_c = nu_peak, nu_m, nu_c
    return o


# ---- link 3: the break frequencies (syn_freq, syn_I_peak) ----
def link3(gamma_m, gamma_c, gamma_a, gamma_M, column_den, Bf, B=DEFAULT):
    """dict of nu_m, nu_c, nu_a, nu_M, I_nu_max from the stored electrons: _mathref.breaks_from_physical."""
    return dict(zip(("nu_m", "nu_c", "nu_a", "nu_M", "I_nu_max"), mr.breaks_from_physical(gamma_m, gamma_c, gamma_a, gamma_M, column_den, Bf, B)))


# ---- unshocked cells ----
def unshocked_cell(p):
    """The eleven outputs of a cell with Gamma_th = 1, B = 0, N_p = 0 (t_comv, r > 0), by class: a value, +inf or NaN.

    compute_syn_gamma_M returns +inf for B == 0 and compute_syn_freq returns 0 for B == 0 whatever gamma is: gamma_M = inf, every nu = 0.
    gamma_bar ~ 1 / (B^2 t_comv) = inf: gamma_c = inf.  gamma_ave - 1 = 0: gamma_m - 1 = 0 for p > 2 ((p-2)/(p-1) x 0) and for p < 2
    ((c x 0 x inf^(p-2))^(1/(p-1)) = 0), so f_syn = 0 / 1 = 0 (0^((p-1)/2) = 0 for p > 3) and N_e = column_den = I_peak = 0.  For p == 2
    the bisection starts from the bracket [0, gamma_M = inf], whose stop test inf > inf is false at once: gamma_m - 1 = (0 + inf) / 2 = inf,
    f_syn = inf / inf = NaN and N_e, column_den, I_nu_max are NaN.  gamma_a: kT ~ (gamma_peak - 1) = 0 (inf for p == 2) and nu_peak = 0,
    so the first form is (0 x c^2 / (0 x 0))^0.6 = NaN (NaN / inf for p == 2), no comparison holds, and gamma_a = sqrt(k NaN / 0) + 1 =
    NaN."""
    nan, inf = float("nan"), float("inf")
    if p == 2:
        v = dict(gamma_m=inf, gamma_c=inf, gamma_a=nan, gamma_M=inf, N_e=nan, column_den=nan, I_nu_max=nan)
    else:
        v = dict(gamma_m=1.0, gamma_c=inf, gamma_a=nan, gamma_M=inf, N_e=0.0, column_den=0.0, I_nu_max=0.0)
    v.update(nu_m=0.0, nu_c=0.0, nu_a=0.0, nu_M=0.0)
    return np.array([v[n] for n in OUT_NAMES])


def same_class(got, want):
    """Equal by class and position: NaN where NaN, the same infinity, the same value elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.array_equal(got, want, equal_nan=True))


# ---- the probe's inputs (VAG_MATH_ELEC_CELL rows: t_comv, r, Gamma_th, B, N_p, eps_e, p, xi_e, relic, inj.gamma_M, inj.gamma_m, inj.gamma_c) ----
PS = (1.7, 2.0, 2.3, 3.0, 3.4)
N_RANDOM, N_RELIC, SEED = 4096, 256, 20261019
K_GAMMA_M = 6 * mr.C_PI * mr.C_E / C_SIGMAT            # gamma_M^2 B
K_GAMMA_BAR = 6 * mr.C_PI * C_ME * mr.C_C / C_SIGMAT   # gamma_bar B^2 t_comv


def nudge(x, k):
    """x moved by k ulps (k may be negative), elementwise."""
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def rows_for(p, dm, dc, Bf, N_p, r, eps_e, xi_e):
    """Probe rows (non-relic) whose gamma_m - 1 and gamma_c - 1 come out near dm and dc: Gamma_th - 1 and t_comv inverted in double."""
    n = dm.size
    gM = np.sqrt(K_GAMMA_M / Bf)
    if p > 2:
        gave = dm * (p - 1) / (p - 2)
    elif p < 2:
        gave = dm ** (p - 1) * (p - 1) / (2 - p) * gM ** (2 - p)
    else:  # root_bisect ends on the equation's UPPER root, gamma_M / k with gave = (gamma_M / k) ln k: near gamma_M whatever gave is, and
        gave = np.minimum(dm, 0.3 * gM)  # none above gave ~ 0.37 gamma_M (gamma_m - 1 underflows to 0 there).  So gamma_m comes out as it does.
    Gth = 1 + gave * xi_e / (eps_e * (C_MP / C_ME))
    t_comv = K_GAMMA_BAR / (Bf * Bf * (dc * (dc + 2) / (dc + 1)))  # gamma_c - 1 / gamma_c = gamma_bar
    z = np.zeros(n)
    return np.stack([t_comv, r, Gth, Bf, N_p, eps_e, np.full(n, p), xi_e, z, z, z + 1, z], axis=1)


def random_rows(p, n, rng):
    return rows_for(p, _logu(rng, 1e-9, 1e6, n), _logu(rng, 1e-9, 1e8, n), _logu(rng, 1e-8, 1e4, n), _logu(rng, 1e30, 1e60, n),
                    _logu(rng, 1.0, 1e8, n), rng.choice([0.3, 0.01], n), rng.choice([1.0, 0.1], n))


def relic_rows(p, n, rng, gamma_m_of):
    """Relic rows: the cell from one draw, the crossing cell's electrons from a second one, scaled so that the cooled gamma_c - 1 stays
    inside [1e-9, 1e8] (gamma_m_of(rows): this cell's gamma_m as doubles, which the cooling scales with)."""
    rows = random_rows(p, n, rng)
    gm = gamma_m_of(rows)
    dc = _logu(rng, 1e-9, 1e8, n)
    inj_dm = (gm - 1) * 10.0 ** rng.uniform(-3, 3, n)
    rows[:, 8] = 1.0
    rows[:, 9] = np.sqrt(K_GAMMA_M / _logu(rng, 1e-8, 1e4, n)) * (1 + inj_dm)  # above the crossing cell's gamma_m
    rows[:, 10] = 1 + inj_dm
    rows[:, 11] = 1 + dc * inj_dm / (gm - 1)
    return rows


# ---- a float64 restatement of the chain in the producers' operation order, pow as exp2(b log2 a) as fast_pow does.  It shows what IEEE
#      double gives on these formulas (attainability), carries the deliberate defects of the sensitivity checks (`mut`), and places the
#      probe's inputs. ----
MUTATIONS = ("p4_in_fast_double_break", "gamma_a_without_plus_1", "peak_is_gamma_m", "f_syn_not_raised", "p_below_2_form", "relic_gamma_M_uncooled")


def _fpow(a, b):
    return np.exp2(b * np.log2(a))


def f64_elec_basic(t_comv, Gth, Bf, eps_e, p, xi_e, mut=()):
    with np.errstate(all="ignore"):
        gM = np.where(Bf == 0, np.inf, np.sqrt(K_GAMMA_M / (Bf * (1 + 0.))))
        gave = eps_e * (Gth - 1) * (C_MP / C_ME) / xi_e
        hi = (p - 2) / (p - 1) * gave
        lo = _fpow((2 - p) / (p - 1) * gave * _fpow(gM, p - 2), 1 / (p - 1))
        gm_m1 = np.where((p > 2) & ("p_below_2_form" not in mut), hi, lo)
        two = np.flatnonzero(p == 2)
        if two.size:  # root_bisect
            g, a = gM[two], gave[two]
            eq = lambda x: x * np.log(g) - (x + 1) * np.log(x) - a - np.log(g)  # noqa: E731
            low, high = np.zeros(two.size), g.copy()
            for _ in range(1000):
                act = (high - low) > np.abs((high + low) * 0.5) * P2_STOP
                if not act.any():
                    break
                mid = 0.5 * (high + low)
                up = eq(mid) * eq(high) > 0
                high = np.where(act & up, mid, high)
                low = np.where(act & ~up, mid, low)
            gm_m1[two] = 0.5 * (high + low)
        gbar = K_GAMMA_BAR / (Bf * Bf * (1 + 0.) * t_comv) * 1
        return gM, gm_m1 + 1, (gbar + np.sqrt(gbar * gbar + 4)) / 2


def _f64_freq(g, Bf):
    return np.where((Bf == 0) | ~np.isfinite(g), 0.0, mr.K_SYN_FREQ * Bf * g * g)


def f64_cell(rows, mut=()):
    """syn_cell on probe rows: (out [n][11] in OUT_NAMES order, nu_a of link 2 [n], branch [n])."""
    rows = np.asarray(rows, dtype=np.float64)
    t_comv, r, Gth, Bf, N_p, eps_e, p, xi_e, relic, iM, im, ic = rows.T
    relic = relic != 0
    with np.errstate(all="ignore"):
        gM, gm, gc = f64_elec_basic(t_comv, Gth, Bf, eps_e, p, xi_e, mut)
        f = (gm - 1) / gm
        if "f_syn_not_raised" not in mut:
            f = np.where(p > 3, _fpow(f, (p - 1) / 2), f)
        N_e = N_p * xi_e * f
        cd = N_e / (r * r)
        I = Bf * mr.K_SYN_P * cd / (4 * mr.C_PI)
        ad = (gm - 1) / (im - 1)
        gc = np.where(relic, (ic - 1) * ad + 1, gc)
        if "relic_gamma_M_uncooled" not in mut:
            gM = np.where(relic, (iM - 1) * ad + 1, gM)
        g_peak = gm if "peak_is_gamma_m" in mut else np.where(gc < gm, gc, gm)
        nu_peak, nu_m, nu_c = _f64_freq(g_peak, Bf), _f64_freq(gm, Bf), _f64_freq(gc, Bf)
        kT = (g_peak - 1) * (C_ME * mr.C_C2) / 3
        x = I * mr.C_C2 / (2 * kT)
        db = _fpow(x * np.sqrt(nu_c) * _fpow(nu_m, p / 2), 2 / (p + 5))
        db_fast = _fpow(x * np.sqrt(nu_c) * _fpow(nu_m, p / 2), 2 / (p + 4)) if "p4_in_fast_double_break" in mut else db
        n0 = _fpow(I * mr.C_C2 / (np.cbrt(nu_peak) * 2 * kT), 0.6)
        n1 = _fpow(x * _fpow(nu_m, p / 2), 2 / (p + 4))
        n3 = _fpow(x * np.sqrt(nu_c), 0.4)
        above, slow = n0 > nu_peak, gc > gm
        branch = np.where(~above, 0, np.where(slow, np.where(n1 > nu_c, 2, 1), np.where(n3 > nu_m, 4, 3)))
        nu_a2 = np.choose(branch, [n0, n1, db, n3, db_fast])
        ga = np.sqrt((4 * mr.C_PI * C_ME * mr.C_C / (3 * mr.C_E)) * (nu_a2 / Bf)) + (0 if "gamma_a_without_plus_1" in mut else 1)
        out = np.stack([gm, gc, ga, gM, N_e, cd, _f64_freq(gm, Bf), _f64_freq(gc, Bf), _f64_freq(ga, Bf), _f64_freq(gM, Bf),
                        Bf * mr.K_SYN_P * cd / (4 * mr.C_PI)], axis=1)
    return out, nu_a2, branch


def f64_fwd_state(rows):
    """fwd_shock_state on VAG_MATH_FWD_STATE rows {Gamma, rho, U, m2, eps_B}: [n][4] = Gamma_th, B, N_p, compression."""
    G, rho, U, m2, eps_B = np.asarray(rows, dtype=np.float64).T
    with np.errstate(all="ignore"):
        g = np.where(G - 1 <= 0, 1.0, 1 + (1 - G) * (1 - G) / (G - 1))
        ad = 4.0 / 3.0 + 1 / (3 * g)
        u_down = np.sqrt(np.maximum((g - 1) * (ad - 1) * (ad - 1) / (-ad * (ad - 2) * (g - 1) + 2), 0.0))
        u_up = np.sqrt((1 + u_down * u_down) * np.maximum((g - 1) * (g + 1), 0.0)) + u_down * g
        comp = np.where(u_down == 0, 4 * g, u_up / u_down)
        Gth = U / (m2 * mr.C_C2) + 1
        Bf = np.sqrt(8 * mr.C_PI * eps_B * ((Gth - 1) * (rho * comp) * mr.C_C2))
        sh = m2 != 0
        return np.stack([np.where(sh, Gth, 1.0), np.where(sh, Bf, 0.0), np.where(sh, m2 / C_MP, 0.0), np.where(sh, comp, 0.0)], axis=1)


# ---- the probe's input set ----
UNSHOCKED_ROW = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.1, 2.3, 1.0, 0, 0, 1, 0])
N_PLACED = 16  # base cells per threshold, each at nudge(., -2 ... 2)
KS = (-2, -1, 0, 1, 2)


def _gm_f64(rows):
    return f64_cell(rows)[0][:, 0]


def _placed_on_nu_a(rows, which):
    """Rows whose N_p is scaled so that a nu_a form meets its threshold -- "peak": form 0 = nu_peak; "c": form 1 = nu_c (slow cooling);
    "m": form 3 = nu_m (fast cooling) -- then moved by -2 ... 2 ulps.  nu_a ~ N_p^e with e = 0.6, 2 / (p + 4), 0.4."""
    out, _, _ = f64_cell(rows)
    l2 = link2(out[:, 0], out[:, 1], rows[:, 3], rows[:, 4], rows[:, 1], rows[:, 6], rows[:, 7])
    slow = l2.slow
    form, thr, e, keep = {"peak": (0, l2.nu_peak, 0.6, np.ones_like(slow)), "c": (1, l2.nu_c, 2 / (rows[:, 6] + 4), slow),
                          "m": (3, l2.nu_m, 0.4, ~slow)}[which]
    scale = mr.to_float(_pow(DEFAULT, thr / l2.nu_a_forms[form], mr._in(DEFAULT, 1 / np.asarray(e) + 0 * rows[:, 6])))
    ok = np.flatnonzero(keep & np.isfinite(scale) & (scale > 0))[:N_PLACED]
    base = rows[ok].copy()
    base[:, 4] *= scale[ok]
    return np.concatenate([np.column_stack([base[:, :4], nudge(base[:, 4], k), base[:, 5:]]) for k in KS])


def _placed_gamma_c_on_gamma_m(rows):
    """Relic rows whose cooled gamma_c lands on gamma_m +- 2 ulps: the crossing cell's gamma_m is this cell's own, its gamma_c that moved
    by k ulps."""
    base = rows[:N_PLACED].copy()
    gm = _gm_f64(base)
    res = []
    for k in KS:
        b = base.copy()
        b[:, 8], b[:, 9], b[:, 10], b[:, 11] = 1.0, 1e3 * gm, gm, nudge(gm, k)
        res.append(b)
    return np.concatenate(res)


def _steered(rows, rng):
    """Rows whose N_p puts nu_a between nu_m and nu_c in slow cooling (branch 1: form 1 ~ N_p^(2/(p+4))), above nu_c there (branch 2),
    and above nu_m in fast cooling (branch 4: form 3 ~ N_p^0.4)."""
    out, _, _ = f64_cell(rows)
    l2 = link2(out[:, 0], out[:, 1], rows[:, 3], rows[:, 4], rows[:, 1], rows[:, 6], rows[:, 7])
    lc, lm = DEFAULT.log2(l2.nu_c), DEFAULT.log2(l2.nu_m)
    decade = DEFAULT.log2(DEFAULT.const(10.0))
    res = []
    for form, slow, lo, hi, within in ((1, True, 0.05, 0.95, True), (1, True, 0.1, 3.0, False), (3, False, 0.1, 3.0, False)):
        u = mr._in(DEFAULT, rng.uniform(lo, hi, rows.shape[0]))
        target = DEFAULT.exp2(lm + u * (lc - lm)) if within else DEFAULT.exp2((lc if slow else lm) + u * decade)
        inv_e = (rows[:, 6] + 4) / 2 if form == 1 else np.full(rows.shape[0], 2.5)
        scale = mr.to_float(_pow(DEFAULT, target / l2.nu_a_forms[form], mr._in(DEFAULT, inv_e)))
        ok = np.flatnonzero((l2.slow == slow) & (np.abs(mr.to_float(lc - lm)) > 0.1) & np.isfinite(scale) & (scale > 0))[:N_STEERED]
        b = rows[ok].copy()
        b[:, 4] *= scale[ok]
        res.append(b)
    return np.concatenate(res)


N_STEERED = 160
_SETS = {}


def probe_set(p):
    """(rows [n][12], kind [n]) for one of PS: "random", "relic", "placed" (on a threshold), "steered" (p = 2: drawn like "random", N_p moved into
    branches 1, 2 and 4), "unshocked", "p-ulp" (p one ulp either side of
    2 or 3, with the p = 2.0 and p = 3.0 sets).  One fixed seed; cached."""
    if p in _SETS:
        return _SETS[p]
    rng = np.random.default_rng([SEED, int(round(p * 10))])
    parts = [("random", random_rows(p, N_RANDOM, rng)), ("relic", relic_rows(p, N_RELIC, rng, _gm_f64))]
    src = random_rows(p, 2048, rng)
    placed = [_placed_on_nu_a(src, w) for w in ("peak", "c", "m")] + [_placed_gamma_c_on_gamma_m(src)]
    parts.append(("placed", np.concatenate(placed)))
    if p == 2:  # gamma_m ~ gamma_M here (rows_for): the plain draw leaves the absorbed branches 1, 2 and 4 nearly empty, so N_p is steered there
        parts.append(("steered", _steered(random_rows(p, 2048, rng), rng)))
    un = UNSHOCKED_ROW.copy()
    un[6] = p
    parts.append(("unshocked", un[None]))
    if p in (2.0, 3.0):
        for k in (-1, 1):
            q = float(nudge(p, k))
            parts.append(("p-ulp", random_rows(q, 64, rng)))
            parts.append(("p-ulp", relic_rows(q, 16, rng, _gm_f64)))
    rows = np.concatenate([r for _, r in parts])
    kind = np.concatenate([np.full(r.shape[0], k) for k, r in parts])
    _SETS[p] = (rows, kind)
    return _SETS[p]


def fwd_state_rows(n=4096, seed=SEED):
    """VAG_MATH_FWD_STATE rows: Gamma - 1 in [1e-9, 1e3] (+ Gamma = 1 exactly and below), rho, m2 log-uniform, Gamma_th - 1 in [1e-9, 1e3]
    through U, eps_B in [1e-6, 0.5]; the last row is unshocked (m2 = 0)."""
    rng = np.random.default_rng([seed, 0])
    G = 1 + _logu(rng, 1e-9, 1e3, n)
    G[:4] = [1.0, 1 - 2.0 ** -53, 1 + 2.0 ** -52, 0.5]
    m2 = _logu(rng, 1e-20, 1e5, n)
    rows = np.stack([G, _logu(rng, 1e-15, 1e10, n), _logu(rng, 1e-9, 1e3, n) * m2, m2, _logu(rng, 1e-6, 0.5, n)], axis=1)
    rows[-1, 3] = 0.0
    return rows


# ---- ceilings: conditions, not measurements.  Each is about 25 x what IEEE double with glibc's exp2 / log2 / cbrt gives on the same formula
#      (tests/test_electron_stage_host.py measures those figures on the float64 restatement and asserts them under the ceilings). ----
def ceiling(link, name, pcls):
    if link == 0:
        # measured on the restatement: compression 6.2e-16, Gamma_th 1.6e-16, N_p 1.1e-16, B 2.3e-16; 25 x the largest is 1.6e-14 (the
        # device's rcp_fast and sqrt_fast are within 2 ulp each, the size of the IEEE operations they stand for)
        return 2e-14
    if link == 2 and name in ("gamma_a", "nu_a"):
        return 5e-13  # pows of arguments up to 2^+-100
    if (link == 1 and name == "gamma_m" and pcls == "p<2") or (link == 2 and name in ("N_e", "column_den", "I_nu_max") and pcls == "p>3"):
        return 1e-13  # two pows / f_syn raised to a power
    return 2e-14


def chain_errors(t_comv, r, Gamma_th, Bf, N_p, eps_e, p, xi_e, out, relic=None, inj=None, B=DEFAULT):
    """Links 1-3 on one producer's outputs (`out`: name -> doubles [n], OUT_NAMES; "column_den" may be missing), every link fed with the
    producer's own doubles of the link before.  All arguments are [n] doubles of SHOCKED cells in code units (p, eps_e, xi_e broadcast);
    relic [n] bool with inj = (gamma_M, gamma_m, gamma_c) [n] of the crossing cell.  Returns {(link, name): relative error [n]} -- NaN
    where a quantity has no reference (gamma_m at p == 2) -- and "link2" (the Link2 of the cells), "p2_ok" [n] (True off p == 2)."""
    n = np.size(Bf)
    p, eps_e, xi_e = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (p, eps_e, xi_e))
    relic = np.zeros(n, dtype=bool) if relic is None else np.asarray(relic, dtype=bool)
    e = {}
    with np.errstate(all="ignore"):
        gM, gm, gc = link1(t_comv, Gamma_th, Bf, eps_e, p, xi_e, B)
        if relic.any():
            iM, im, ic = (np.where(relic, v, 2.0) for v in inj)
            rM, rc = link1_relic(iM, im, ic, out["gamma_m"], B)
            gM, gc = mr._where(relic, rM, gM), mr._where(relic, rc, gc)
        e[1, "gamma_M"], e[1, "gamma_m"], e[1, "gamma_c"] = rel(out["gamma_M"], gM), rel(out["gamma_m"], gm), rel(out["gamma_c"], gc)
        two = p == 2
        ok = np.ones(n, dtype=bool)
        if two.any():
            ok[two] = p2_bracket_holds(out["gamma_m"][two], np.asarray(Gamma_th)[two], np.asarray(Bf)[two], eps_e[two], xi_e[two], B)
        l2 = link2(out["gamma_m"], out["gamma_c"], Bf, N_p, r, p, xi_e, B)
        e[2, "N_e"], e[2, "I_nu_max"] = rel(out["N_e"], l2.N_e), rel(out["I_nu_max"], l2.I_peak)
        e[2, "gamma_a"], _ = l2.nearest(l2.gamma_a_forms, out["gamma_a"])
        cd = out.get("column_den")
        if cd is not None:
            e[2, "column_den"] = rel(cd, l2.column_den)
        l3 = link3(out["gamma_m"], out["gamma_c"], out["gamma_a"], out["gamma_M"], np.ones(n) if cd is None else cd, Bf, B)
        for name in ("nu_m", "nu_c", "nu_a", "nu_M") + (() if cd is None else ("I_nu_max",)):
            e[3, name] = rel(out[name], l3[name])
    e["link2"], e["p2_ok"] = l2, ok
    return e


def worst_by_class(errs, p, select=None):
    """{(link, name, p class): max error} over the selected cells, NaN entries (no reference) left out."""
    p = np.asarray(p, dtype=np.float64)
    cls = np.array([pclass(v) for v in p])
    res = {}
    for key, v in errs.items():
        if not isinstance(key, tuple):
            continue
        for c in np.unique(cls):
            m = (cls == c) & ~np.isnan(v) & (True if select is None else select)
            if m.any():
                res[key + (str(c),)] = float(np.max(v[m]))
    return res


RELIC_SEEN = 1e-9  # a relic cell's gamma_c is off the synchrotron-only form by its cooling history (per cent); a fresh cell's by ~1e-16


def injection_index(t_comv, Bf, gamma_c, B=DEFAULT):
    """Per row of [rows][n_t] arrays: the first cell whose gamma_c is not the synchrotron-only form of link 1 (n_t: none).  Cells with
    B == 0 are passed over."""
    with np.errstate(all="ignore"):
        gbar = _k(B, (6, mr.C_PI, C_ME, mr.C_C), (C_SIGMAT,)) / (mr._in(B, Bf) * mr._in(B, Bf) * mr._in(B, t_comv))
        off = rel(gamma_c, (gbar + B.sqrt(gbar * gbar + 4)) / 2) > RELIC_SEEN
    off &= np.asarray(Bf) != 0
    return np.where(off.any(axis=1), off.argmax(axis=1), off.shape[1])


def details_errors(cells, out, rad, rvs, B=DEFAULT):
    """Links 1-3 on the [n_theta][n_t] arrays of one shock's details call: cells = {t_comv, r, Gamma_th, B, N_p} and out = {OUT_NAMES}
    (column_den may be missing) in code units, rad = {p, eps_e, xi_e} of that shock.  Every row of a reverse shock (`rvs`) has one
    injection index k_inj (injection_index): cells below it follow the synchrotron-only link 1, cells from it on the relic form with the
    electrons of cell k_inj - 1.  Unshocked cells (B == 0) are compared with `unshocked_cell` by class; cells whose gamma_peak is exactly
    1 (kT = 0: nu_a is not defined) are counted and left out.  Returns n, n_unshocked, n_relic, n_degenerate, k_inj [n_theta], worst
    {(link, name, p class): max error}, errors (chain_errors of the compared cells) and `index` (their flat positions)."""
    Bf = np.asarray(cells["B"], dtype=np.float64)
    nth, nt = Bf.shape
    k_inj = injection_index(cells["t_comv"], Bf, out["gamma_c"], B) if rvs else np.full(nth, nt)
    relic = np.arange(nt)[None, :] >= k_inj[:, None]
    src = np.clip(k_inj - 1, 0, nt - 1)
    inj = tuple(np.broadcast_to(out[n][np.arange(nth), src][:, None], Bf.shape) for n in ("gamma_M", "gamma_m", "gamma_c"))
    unshocked = Bf == 0
    want = unshocked_cell(rad["p"])
    for i, n in enumerate(OUT_NAMES):
        if n in out and unshocked.any():
            v = out[n][unshocked]
            assert same_class(v, np.full(v.shape, want[i])), f"unshocked cells: {n} is not {want[i]}"
    degenerate = ~unshocked & (np.minimum(out["gamma_m"], out["gamma_c"]) == 1)
    sel = ~unshocked & ~degenerate
    f = lambda a: np.asarray(a, dtype=np.float64)[sel]  # noqa: E731
    errs = chain_errors(f(cells["t_comv"]), f(cells["r"]), f(cells["Gamma_th"]), f(Bf), f(cells["N_p"]), rad["eps_e"], rad["p"], rad["xi_e"],
                        {n: f(v) for n, v in out.items()}, relic[sel], tuple(v[sel] for v in inj), B)
    return dict(n=Bf.size, n_unshocked=int(unshocked.sum()), n_relic=int((relic & sel).sum()), n_degenerate=int(degenerate.sum()), k_inj=k_inj,
                worst=worst_by_class(errs, np.full(int(sel.sum()), rad["p"])), errors=errs, index=np.flatnonzero(sel), p2_ok=bool(np.all(errs["p2_ok"])))
