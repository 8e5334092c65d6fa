"""Extended-precision reference of what lies between the pair solver's raw ODE state and the reverse-shock cells (Gamma_th, B, N_p) the
electron stage reads (tests/test_reverse_state_host.py, tests/test_reverse_state.py).  Device: vag_rs.h -- the closed forms rel_Gamma,
downstr_4vel, jump_4vel, sound_speed and their fast forms, rvs_shock_state, rvs_cross_state, rvs_early_extrap, CrossLattice and
PairShock::init_state; the reference's sources are the ones vag_rs.h cites beside each.  The ODE right-hand side and the integrator are
not here: they are held end to end only.

Every routine is restated three times:
* `ref_*`: the formula in numpy.longdouble on the float64 inputs taken exactly; the cubic of the magnetised jump in mpmath at CUBIC_DPS
  digits (the trigonometric solution loses ~2 x log10(1 / (gamma_rel - 1)) digits to cancellation) with the device's selection rule:
  x_max the largest real root, u_down^2 the larger of the other two, 0 where x_max <= 0;
* `f64_*`: the same in float64 in the device's statement order -- what IEEE double with the C library gives on the formula, the figure
  the ceilings come from -- carrying the deliberate defects of the sensitivity checks (`mut`);
* `f64_*_f`: the fast forms with an exact reciprocal and square root, each call perturbed by +- the project's figures for rcp1 (2.2e-15)
  and sqrt1 (4.2e-15): the bound on |fast - exact|.

Thresholds.  A comparison of a COMPUTED value with a threshold (sigma of the state against SIGMA_CUT, Gamma_th against GAMMA_CUT,
Gamma34 > 1, denom <= 0, t_refine against ts and t_end, the truncation to an integer of the lattice's n_post) is decided exactly and,
where the value is within two roundings (NEAR = 2^-52, relative to the operands before they cancel) of the threshold, both ways: the
`admitted` generator yields every reference some decision reaches and `nearest` compares a produced value with the nearest one.  A
comparison of an INPUT double with a threshold (sigma handed to downstr_4vel, t0 < T0, Gamma_th of an extrapolation row) involves no
rounding and is decided exactly: `sigma < SIGMA_CUT` for `<=` is a defect the reference sees.

Metric: the relative error of the returned value (0 against 0 is no error).  For rel_Gamma that is Gamma34, not Gamma34 - 1: the device
returns 1 + d^2 / denom as the reference source does, and Gamma34 - 1 formed from that double has lost its digits below 1e-16.  Where a
later quantity is formed from such a stored double (U3 = (Gamma34 - 1) m3 c^2 of init_state) the reference forms it from the double the
producer must have stored -- the correctly rounded Gamma34 or a neighbour -- as tests/_elecref.py feeds every link the stored doubles.

Everything is in the engine's code units (_mathref's constants)."""
import itertools

import numpy as np

import _mathref as mr

mpmath = mr.mpmath
LDT = np.longdouble
SIGMA_CUT = 1e-6
GAMMA_CUT = 1.0 + 1e-6
RS_SEED_FRAC = 1e-8
C_C2, C_MP, C_PI = mr.C_C2, mr.C_MP, mr.C_PI
NEAR = 2.0 ** -52
CUBIC_DPS = 100
E_RCP1, E_SQRT1 = 2.2e-15, 4.2e-15  # tests/test_device_math.py holds rcp1 and sqrt1 to these
SEED = 20261021
N_RANDOM = 4096
MEDIUM_ISM, MEDIUM_WIND = 0, 1
LOG2_10 = 3.321928094887362347870319429489390175865

MUTATIONS = ("vieta_other_root", "sigma_lt_cut", "rel_gamma_no_u1u2", "ad_four_thirds", "post_compression_inverted", "limiter_after_crossing",
             "slope_from_next_node", "n_pre_without_shared_node", "second_segment_node0_twice", "gamma_th_with_m4")


def ld(x):
    return np.asarray(x, dtype=np.float64).astype(LDT)


def rel(got, ref):
    """|got - ref| / |ref| as float64; 0 where both are 0, inf where only the reference is."""
    got, ref = np.asarray(got, dtype=np.float64).astype(LDT), np.asarray(ref, dtype=LDT)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / np.abs(ref)
    e = np.where(ref == 0, np.where(got == 0, 0.0, np.inf), e)
    return np.where(np.isnan(e), np.inf, e).astype(np.float64)


def nudge(x, k):
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _gt(v, t, scale, side):
    """v > t; within NEAR x scale of t decided as if on `side` of it (None: exactly)."""
    c = np.asarray(v > t, dtype=bool)
    if side is None:
        return c
    near = np.abs((v - t).astype(np.float64)) <= NEAR * np.asarray(scale, dtype=np.float64)
    return np.where(near, side > 0, c)


def admitted(fn, names):
    """fn(side) for the exact decisions and for every way of deciding the named thresholds where they are near (`side`: name -> -1 / +1,
    a missing name is decided exactly)."""
    yield fn({})
    for combo in itertools.product((-1, 1), repeat=len(names)):
        yield fn(dict(zip(names, combo)))


def nearest(got, refs):
    """Per element the relative distance of `got` from the nearest of the references."""
    return np.minimum.reduce([rel(got, r) for r in refs])


# ================================================================ the closed forms
def _ad(g):
    return LDT(4) / 3 + 1 / (3 * g)


def ref_rel_Gamma(g1, g2, side=None):
    g1, g2 = ld(g1) if np.asarray(g1).dtype != LDT else g1, ld(g2) if np.asarray(g2).dtype != LDT else g2
    u1u2 = np.sqrt(np.maximum((g1 - 1) * (g1 + 1) * (g2 - 1) * (g2 + 1), 0))
    d = g1 - g2
    denom = g1 * g2 - 1 + u1u2
    pos = _gt(denom, 0, g1 * g2, None if side is None else side.get("denom"))
    return np.where(pos, 1 + d * d / np.where(denom == 0, 1, denom), LDT(1))


def _mp(v):
    """A longdouble (or double) as an mpf, exactly."""
    v = LDT(v)
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - LDT(hi)))


def _from_mp(v):
    hi = float(v)
    return LDT(hi) + LDT(float(v - mpmath.mpf(hi)))


def cubic_coefficients(g, sigma):
    """(b, c, d) of x^3 + b x^2 + c x + d = 0 for x = u_down^2 (compute_downstr_4vel, shock.cpp:93-137), in mpmath."""
    ad = mpmath.mpf(4) / 3 + 1 / (3 * g)
    gm1, adm2, adm1, g2, gp1 = g - 1, ad - 2, ad - 1, g * g, g + 1
    term1, term2 = -ad * adm2, g2 - 1
    A = term1 * gm1 + 2
    B = -gp1 * (-adm2 * (ad * g2 + 1) + ad * adm1 * g) * sigma - gm1 * (term1 * (g2 - 2) + 2 * g + 3)
    Cc = gp1 * (ad * (1 - ad / 4) * term2 + 1) * sigma * sigma + term2 * (2 * g + adm2 * (ad * g - 1)) * sigma + gp1 * gm1 * gm1 * adm1 * adm1
    D = -gm1 * gp1 * gp1 * adm2 * adm2 * sigma * sigma / 4
    return B / A, Cc / A, D / A


def cubic_u_down_mp(g, sigma):
    """u_down of the magnetised jump for one (gamma_rel, sigma), mpmath values in and out (call under mpmath.workdps(CUBIC_DPS))."""
    b, c, d = cubic_coefficients(g, sigma)
    P = c - b * b / 3
    Q = 2 * b * b * b / 27 - b * c / 3 + d
    u = mpmath.sqrt(max(-P, 0) / 3)
    den = 2 * P * u
    v = min(max(3 * Q / den, -1), 1) if den != 0 else mpmath.mpf(0)
    phi = mpmath.acos(v)
    roots = sorted(2 * u * mpmath.cos((phi - 2 * mpmath.pi * k) / 3) - b / 3 for k in range(3))
    x_max = roots[2]
    if x_max <= 0:
        return mpmath.mpf(0)
    return mpmath.sqrt(max(roots[1], 0))


_CUBIC = {}


def ref_cubic_u_down(g, sigma):
    """u_down [n] (longdouble) of the cubic branch, g and sigma longdouble or double arrays; cached per point."""
    g, sigma = np.atleast_1d(np.asarray(g, dtype=LDT)), np.atleast_1d(np.asarray(sigma, dtype=LDT))
    out = np.empty(g.shape, dtype=LDT)
    with mpmath.workdps(CUBIC_DPS):
        for i in range(g.size):
            key = (g[i].tobytes(), sigma[i].tobytes())
            if key not in _CUBIC:
                _CUBIC[key] = _from_mp(cubic_u_down_mp(_mp(g[i]), _mp(sigma[i])))
            out[i] = _CUBIC[key]
    return out


def ref_downstr_4vel(g, sigma, mag=None):
    """u_down; `mag` [n] bool: the points that take the cubic (default: sigma > SIGMA_CUT, decided exactly)."""
    g, sigma = np.asarray(g, dtype=LDT), np.asarray(sigma, dtype=LDT)
    g, sigma = np.broadcast_arrays(g, sigma)
    mag = np.asarray(sigma > LDT(SIGMA_CUT), dtype=bool) if mag is None else np.broadcast_to(mag, g.shape)
    ad = _ad(g)
    gm1 = g - 1
    out = np.sqrt(np.maximum(gm1 * (ad - 1) * (ad - 1) / (-ad * (ad - 2) * gm1 + 2), 0))
    if mag.any():
        out = out.copy()
        out[mag] = ref_cubic_u_down(g[mag], sigma[mag])
    return out


def ref_jump_4vel(g, sigma, mag=None):
    g, sigma = np.asarray(g, dtype=LDT), np.asarray(sigma, dtype=LDT)
    ud = ref_downstr_4vel(g, sigma, mag)
    uu = np.sqrt((1 + ud * ud) * np.maximum((g - 1) * (g + 1), 0)) + ud * g
    with np.errstate(all="ignore"):
        return np.where(ud == 0, 4 * g, uu / np.where(ud == 0, 1, ud))


def ref_sound_speed(G):
    G = ld(G)
    ad = _ad(G)
    return np.sqrt(np.maximum(ad * (ad - 1) * (G - 1) / (1 + (G - 1) * ad), 0))


# ---- float64 restatements, the device's statement order ----
class Pert:
    """The exact 1 / x and sqrt(x), call number i moved by signs[i] x the project's figure (no signs: the exact operations)."""

    def __init__(self, signs=()):
        self.signs, self.i = tuple(signs), 0

    def _s(self):
        s = self.signs[self.i] if self.i < len(self.signs) else 0
        self.i += 1
        return s

    def rcp(self, x):
        return (1 / x) * (1 + self._s() * E_RCP1)

    def sqrt(self, x):
        return np.sqrt(x) * (1 + self._s() * E_SQRT1)


def f64_rel_Gamma(g1, g2, mut=(), op=None):
    op = op or Pert()
    with np.errstate(all="ignore"):
        u1u2 = op.sqrt(np.maximum((g1 - 1) * (g1 + 1) * (g2 - 1) * (g2 + 1), 0.0))
        d = g1 - g2
        denom = g1 * g2 - 1 + (0 if "rel_gamma_no_u1u2" in mut else u1u2)
        return np.where(denom <= 0, 1.0, 1 + d * d * op.rcp(denom))


def f64_downstr_4vel(g, sigma, mut=(), ad=None):
    g, sigma = np.broadcast_arrays(np.asarray(g, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    with np.errstate(all="ignore"):
        ad = (np.full(g.shape, 4.0 / 3.0) if "ad_four_thirds" in mut else 4.0 / 3.0 + 1 / (3 * g)) if ad is None else ad
        gm1, adm2, adm1 = g - 1, ad - 2, ad - 1
        hydro = np.sqrt(np.maximum(gm1 * adm1 * adm1 / (-ad * adm2 * gm1 + 2), 0.0))
        g2, gp1 = g * g, g + 1
        term1, term2 = -ad * adm2, g2 - 1
        A = term1 * gm1 + 2
        B = -gp1 * (-adm2 * (ad * g2 + 1) + ad * adm1 * g) * sigma - gm1 * (term1 * (g2 - 2) + 2 * g + 3)
        Cc = gp1 * (ad * (1 - ad / 4) * term2 + 1) * sigma * sigma + term2 * (2 * g + adm2 * (ad * g - 1)) * sigma + gp1 * gm1 * gm1 * adm1 * adm1
        D = -gm1 * gp1 * gp1 * adm2 * adm2 * sigma * sigma / 4
        b, c, d = B / A, Cc / A, D / A
        P = c - b * b / 3
        Q = 2 * b * b * b / 27 - b * c / 3 + d
        u = np.sqrt(np.maximum(-P, 0.0) / 3)
        denom = 2 * P * u
        v = np.where(denom != 0, np.minimum(np.maximum(3 * Q / denom, -1.0), 1.0), 0.0)
        x_max = 2 * u * np.cos(np.arccos(v) / 3) - b / 3
        prod = -d / x_max
        s = (c - prod) / x_max
        root = np.sqrt(np.maximum(s * s - 4 * prod, 0.0))
        uds = (s - root) / 2 if "vieta_other_root" in mut else (s + root) / 2
        cubic = np.where(x_max <= 0, 0.0, np.sqrt(np.maximum(uds, 0.0)))
        take_hydro = sigma < SIGMA_CUT if "sigma_lt_cut" in mut else sigma <= SIGMA_CUT
        return np.where(take_hydro, hydro, cubic)


def f64_jump_4vel(g, sigma, mut=()):
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        ud = f64_downstr_4vel(g, sigma, mut)
        uu = np.sqrt((1 + ud * ud) * np.maximum((g - 1) * (g + 1), 0.0)) + ud * g
        return np.where(ud == 0, 4 * g, uu / ud)


def f64_jump_4vel_f(g, sigma, mut=(), op=None):
    """jump_4vel_f: the hydrodynamic jump on rcp1 / sqrt1 (3 + 2 calls), the exact cubic form where sigma > SIGMA_CUT."""
    op = op or Pert()
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        ad = 4.0 / 3.0 + op.rcp(3 * g)
        if "ad_four_thirds" in mut:
            ad = np.full(g.shape, 4.0 / 3.0)
        gm1, adm2, adm1 = g - 1, ad - 2, ad - 1
        r1 = op.rcp(-ad * adm2 * gm1 + 2)
        ud = op.sqrt(np.maximum(gm1 * adm1 * adm1 * r1, 0.0))
        uu = op.sqrt((1 + ud * ud) * np.maximum(gm1 * (g + 1), 0.0)) + ud * g
        fast = np.where(ud == 0, 4 * g, uu * op.rcp(ud))
        return np.where(np.asarray(sigma) > SIGMA_CUT, f64_jump_4vel(g, sigma, mut), fast)


def f64_sound_speed(G, op=None):
    op = op or Pert()
    G = np.asarray(G, dtype=np.float64)
    with np.errstate(all="ignore"):
        ad = 4.0 / 3.0 + op.rcp(3 * G)
        return op.sqrt(np.maximum(ad * (ad - 1) * (G - 1) * op.rcp(1 + (G - 1) * ad), 0.0))


def fast_bound(fn, n_calls, exact):
    """max over every sign pattern of the n_calls perturbed operations of |fn(op) - exact| / |exact|, per point."""
    worst = np.zeros(np.shape(exact))
    for signs in itertools.product((-1, 1), repeat=n_calls):
        worst = np.maximum(worst, rel(fn(Pert(signs)), ld(exact)))
    return worst


# ================================================================ the cell state
RVS_IN = ("Gamma", "x4", "x3", "m3", "U3", "r", "eps4", "m4", "Gamma4", "eps_B", "crossing", "V3_comv_x", "rho3_x", "B3_ordered_x")
RVS_OUT = ("Gamma_th", "B", "N_p", "V3_comv", "rho3", "B3_ordered")


def _cols(rows, names):
    return {n: rows[:, i] for i, n in enumerate(names)}


def _ref_sigma(eps4, m4, Gamma4, side):
    x = eps4 / (Gamma4 * m4 * LDT(C_C2))
    sigma = x - 1
    mag = _gt(sigma, LDT(SIGMA_CUT), x, None if side is None else side.get("sigma"))
    return np.where(mag, sigma, LDT(0)), mag


def ref_rvs_state(rows, side=None, Gth_stored=None):
    """[n][6] (longdouble) in RVS_OUT order on VAG_MATH_RVS_STATE rows.  side: {"sigma", "gth"} -> -1 / +1.  Gth_stored [n]: the producer's
    own returned Gamma_th, which B is then formed from: Gamma_th - 1 of the stored double is exact, while B formed from U3 / (m3 c^2)
    differs from any double implementation by eps / (Gamma_th - 1) (the convention of tests/_elecref.py link0_B)."""
    side = side or {}
    a = {k: ld(v) for k, v in _cols(np.asarray(rows, dtype=np.float64), RVS_IN).items()}
    crossing = a["crossing"] != 0
    with np.errstate(all="ignore"):
        shocked = a["m3"] != 0
        Gth3 = np.where(shocked, a["U3"] / np.where(shocked, a["m3"] * LDT(C_C2), 1) + 1, LDT(1))
        sigma4, mag = _ref_sigma(a["eps4"], a["m4"], a["Gamma4"], side)
        comp34 = ref_jump_4vel(ref_rel_Gamma(a["Gamma4"], a["Gamma"]), sigma4, mag)
        rho4 = a["m4"] / (a["r"] * a["r"] * a["x4"])
        k4 = LDT(4) * LDT(C_PI) * LDT(C_C2)
        B4 = np.sqrt(k4 * sigma4 * rho4)
        s_gth = side.get("gth")
        kept = ~_gt(LDT(GAMMA_CUT), Gth3, 1.0, None if s_gth is None else -s_gth)  # the limiter drops Gth3 < GAMMA_CUT
        Gth_c = np.where(kept, Gth3, LDT(1))
        Gb_c, Gb_p = (Gth_c, Gth3) if Gth_stored is None else (ld(Gth_stored), ld(Gth_stored))
        B_c = np.sqrt(8 * LDT(C_PI) * a["eps_B"] * ((Gb_c - 1) * (rho4 * comp34) * LDT(C_C2))) + B4 * comp34
        V3 = a["r"] * a["r"] * a["x3"]
        comp = a["V3_comv_x"] / V3
        B_p = np.sqrt(8 * LDT(C_PI) * a["eps_B"] * ((Gb_p - 1) * (a["rho3_x"] * comp) * LDT(C_C2))) + a["B3_ordered_x"] * comp
        return np.stack([np.where(crossing, Gth_c, Gth3), np.where(crossing, B_c, B_p), a["m3"] / LDT(C_MP), V3, rho4 * comp34, B4 * comp34], axis=1)


def f64_rvs_state(rows, mut=()):
    a = _cols(np.asarray(rows, dtype=np.float64), RVS_IN)
    crossing = a["crossing"] != 0
    with np.errstate(all="ignore"):
        m_th = a["m4"] if "gamma_th_with_m4" in mut else a["m3"]
        Gth3 = np.where(a["m3"] == 0, 1.0, a["U3"] * (1 / (m_th * C_C2)) + 1)
        sigma = a["eps4"] / (a["Gamma4"] * a["m4"] * C_C2) - 1
        sigma4 = np.where(sigma > SIGMA_CUT, sigma, 0.0)
        comp34 = f64_jump_4vel_f(f64_rel_Gamma(a["Gamma4"], a["Gamma"], mut), sigma4, mut)
        comp34_x = f64_jump_4vel(f64_rel_Gamma(a["Gamma4"], a["Gamma"], mut), sigma4, mut)
        rho4 = a["m4"] * (1 / (a["r"] * a["r"] * a["x4"]))
        Gth_c = np.where(Gth3 < GAMMA_CUT, 1.0, Gth3)
        B4 = np.where(sigma4 > 0, np.sqrt((4 * C_PI * C_C2) * sigma4 * rho4), 0.0)
        B_c = np.sqrt(8 * C_PI * a["eps_B"] * ((Gth_c - 1) * (rho4 * comp34) * C_C2)) + B4 * comp34
        V3 = a["r"] * a["r"] * a["x3"]
        comp = V3 * (1 / a["V3_comv_x"]) if "post_compression_inverted" in mut else a["V3_comv_x"] * (1 / V3)
        Gth_p = Gth_c if "limiter_after_crossing" in mut else Gth3
        B_p = np.sqrt(8 * C_PI * a["eps_B"] * ((Gth_p - 1) * (a["rho3_x"] * comp) * C_C2)) + a["B3_ordered_x"] * comp
        rho4_x = a["m4"] / (a["r"] * a["r"] * a["x4"])
        return np.stack([np.where(crossing, Gth_c, Gth_p), np.where(crossing, B_c, B_p), a["m3"] / C_MP, V3, rho4_x * comp34_x,
                         np.sqrt((4 * C_PI * C_C2) * sigma4 * rho4_x) * comp34_x], axis=1)


# ================================================================ the lattice
def ref_lattice(ts, t_end, t_dec, T0, t_num, base_t_num, side=None):
    """dict(n_pre, n_post, plain, nodes [t_num] longdouble) of CrossLattice.  side: {"lo", "hi", "np"} -> -1 / +1."""
    side = side or {}
    ts, t_end, t_dec, T0 = (LDT(float(v)) for v in (ts, t_end, t_dec, T0))
    n = int(t_num)
    raw = 10 * max(t_dec, T0)
    t_refine = min(max(raw, ts), t_end)
    s_hi = side.get("hi")
    below = not bool(_gt(raw, ts, raw, side.get("lo")))                           # plain: t_refine <= ts
    above = not bool(_gt(t_end, raw, raw, None if s_hi is None else -s_hi))        # plain: t_refine >= t_end
    l0, l3 = np.log10(ts), np.log10(t_end)
    k = np.arange(n).astype(LDT)
    if below or above:
        nodes = l0 + (l3 - l0) / max(1, n - 1) * k
        nodes[n - 1] = l3
        return dict(n_pre=0, n_post=0, plain=1, nodes=LDT(10) ** nodes)
    lr = np.log10(t_refine)
    x = LDT(int(base_t_num)) * (l3 - lr) / (l3 - l0)
    np_ = int(np.floor(x))
    near_int = abs(float(x - np.round(x))) <= 8 * NEAR * max(1.0, float(x))  # a quotient of two logarithms: a few roundings
    if side.get("np") is not None and near_int:
        np_ = int(np.round(x)) + (0 if side["np"] > 0 else -1)
    if np_ < 2:
        np_ = 2
    if np_ >= n:
        np_ = n // 2
    n_post, n_pre = np_, n + 1 - np_
    nodes = np.empty(n, dtype=LDT)
    nodes[:n_pre] = l0 + (lr - l0) / max(1, n_pre - 1) * k[:n_pre]
    nodes[n_pre - 1] = lr
    q = k[n_pre:] - n_pre + 1
    nodes[n_pre:] = lr + (l3 - lr) / max(1, n_post - 1) * q
    nodes[n - 1] = l3
    return dict(n_pre=n_pre, n_post=n_post, plain=0, nodes=LDT(10) ** nodes)


def f64_lattice(ts, t_end, t_dec, T0, t_num, base_t_num, mut=()):
    n = int(t_num)
    t_refine = min(max(10 * max(t_dec, T0), ts), t_end)
    l0, l3 = np.log10(ts), np.log10(t_end)
    plain = int(t_refine <= ts or t_refine >= t_end)
    step0 = (l3 - l0) / max(1.0, float(n - 1))
    n_pre = n_post = 0
    lr = step1 = step2 = 0.0
    if not plain:
        np_ = int(float(base_t_num) * np.log10(t_end / t_refine) / np.log10(t_end / ts))
        if np_ < 2:
            np_ = 2
        if np_ >= n:
            np_ = n // 2
        n_post = np_
        n_pre = n - n_post if "n_pre_without_shared_node" in mut else n + 1 - n_post
        lr = np.log10(t_refine)
        step1 = (lr - l0) / max(1.0, float(n_pre - 1))
        step2 = (l3 - lr) / max(1.0, float(n_post - 1))
    nodes = np.empty(n)
    for kk in range(n):
        if plain:
            lg = l3 if (n > 1 and kk == n - 1) else l0 + step0 * kk
        elif kk < n_pre:
            lg = lr if (n_pre > 1 and kk == n_pre - 1) else l0 + step1 * kk
        else:
            q = kk - n_pre + (0 if "second_segment_node0_twice" in mut else 1)
            lg = l3 if (n_post > 1 and q == n_post - 1) else lr + step2 * q
        nodes[kk] = np.exp2(lg * LOG2_10)
    return dict(n_pre=n_pre, n_post=n_post, plain=plain, nodes=nodes)


def lattice_variants(lat):
    return list(admitted(lambda s: ref_lattice(*lat, side=s), ("lo", "hi", "np")))


# ================================================================ the early extrapolation
EXT_NODES = 16


def _extrap(rows, LOG2, EXP2, one, slope_node=2):
    """rvs_early_extrap on rows [n][65] -> ([n][16][3], applies [n]); LOG2 / EXP2 / one carry the precision."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    nodes = rows[:, :4 * EXT_NODES].reshape(n, EXT_NODES, 4)
    inj = rows[:, -1].astype(int)
    out = np.array(nodes[:, :, 1:], dtype=type(one))
    applies = np.zeros(n, dtype=bool)
    for i in range(n):
        above = np.flatnonzero(nodes[i, :, 1] > GAMMA_CUT)
        c = int(above[0]) if above.size else EXT_NODES
        if c == 0 or c >= EXT_NODES - 2 or c >= inj[i]:
            continue
        applies[i] = True
        c2 = c + slope_node
        v = np.array(nodes[i], dtype=type(one))
        lr = LOG2(v[:, 0])
        dl = lr[c2] - lr[c]
        for col, off in ((1, one), (2, 0 * one), (3, 0 * one)):
            lc = LOG2(v[c, col] - off)
            slope = (LOG2(v[c2, col] - off) - lc) / dl
            out[i, :c, col - 1] = off + EXP2(lc + slope * (lr[:c] - lr[c]))
    return out, applies


def ref_extrap(rows):
    return _extrap(rows, np.log2, np.exp2, LDT(1))


def f64_extrap(rows, mut=()):
    return _extrap(rows, np.log2, np.exp2, np.float64(1), 1 if "slope_from_next_node" in mut else 2)


# ================================================================ init_state
INIT_IN = ("Gamma4", "deps0_dt", "dm0_dt", "T0", "t0", "eps_e_th", "type", "rho_ism", "A", "r02")
STATE = ("Gamma", "x4", "x3", "m2", "m3", "U2", "U3", "r", "t_comv", "eps4", "m4")


def _simpson(f, u_max):
    """The 32-interval Simpson rule over 18 e-folds below u_max (enclosed_mass_generic, enclosed_thermal_energy_generic)."""
    N = 32
    u_min = u_max - 18
    h = (u_max - u_min) / N
    s = f(u_min) + f(u_max)
    for i in range(1, N, 2):
        s = s + 4 * f(u_min + i * h)
    for i in range(2, N, 2):
        s = s + 2 * f(u_min + i * h)
    return s * h / 3


def _init(rows, T, side=None, g34_nudge=0):
    """PairShock::init_state in the precision of type T (np.float64: the device's statement order; longdouble: the reference) -> [n][11]
    in STATE order.  g34_nudge: the reference forms U3 from the correctly rounded Gamma34 moved by that many ulps."""
    side = side or {}
    exact = T is LDT
    a = {k: np.asarray(v, dtype=np.float64).astype(T) for k, v in _cols(np.asarray(rows, dtype=np.float64), INIT_IN).items()}
    G4, T0, t0 = a["Gamma4"], a["T0"], a["t0"]
    wind = a["type"] == MEDIUM_WIND
    one, c2 = T(1), T(C_C2)
    with np.errstate(all="ignore"):
        rho = lambda r: np.where(wind, a["A"] / (a["r02"] + r * r) + a["rho_ism"], a["rho_ism"])  # noqa: E731
        u4 = np.sqrt((G4 - 1) * (G4 + 1))
        beta4 = u4 / G4
        ad4 = T(4) / 3 + 1 / (3 * G4)
        cs4 = np.sqrt(np.maximum(ad4 * (ad4 - 1) * (G4 - 1) / (1 + (G4 - 1) * ad4), 0))
        r = beta4 * t0 * G4 * G4 * (1 + beta4)
        t_comv = r / u4
        dt = np.minimum(t0, T0)
        eps4, m4 = a["deps0_dt"] * dt, a["dm0_dt"] * dt
        x4 = np.where(t0 < T0, G4 * t0 * beta4, G4 * T0 * beta4 + cs4 * (t0 - T0) * G4)
        u_max = np.log(r)
        m2 = _simpson(lambda u: rho(np.exp(u)) * np.exp(u) * np.exp(u) * np.exp(u), u_max)
        m_jet = a["dm0_dt"] * T0
        Gamma = np.where((m_jet > 0) & (m2 > 0), G4 / (1 + m2 / m_jet), G4)
        ad = T(4) / 3 + 1 / (3 * Gamma)
        ce = 3 * (ad - 1)
        U2 = (1 - a["eps_e_th"]) * (Gamma - 1) * c2 * _simpson(
            lambda u: rho(np.exp(u)) * np.exp(u) * np.exp(u) * np.exp(u) * np.power(np.exp(u) / r, ce), u_max)
        if exact:
            G34 = ref_rel_Gamma(G4, Gamma, side)
            seeded = _gt(G34, one, 1.0, side.get("g34")) & (m4 > 0) & (x4 > 0)
            x = a["deps0_dt"] / (G4 * a["dm0_dt"] * c2)
            sigma = x - 1
            mag = _gt(sigma, T(SIGMA_CUT), x, side.get("sigma"))
            comp = ref_jump_4vel(G34, np.where(mag, sigma, 0), mag)
            G34_stored = nudge(G34.astype(np.float64), g34_nudge).astype(T)
        else:
            G34 = f64_rel_Gamma(G4, Gamma)
            seeded = (G34 > 1) & (m4 > 0) & (x4 > 0)
            sigma = eps4 / (G4 * m4 * c2) - 1
            comp = f64_jump_4vel(G34, np.where(sigma > SIGMA_CUT, sigma, 0.0))
            G34_stored = G34
        x3 = x4 * T(RS_SEED_FRAC)
        m3 = m4 * comp * x3 / x4
        U3 = (G34_stored - 1) * m3 * c2
        z = 0 * x3
        return np.stack([Gamma, x4, np.where(seeded, x3, z), m2, np.where(seeded, m3, z), U2, np.where(seeded, U3, z), r, t_comv, eps4, m4], axis=1)


def ref_init(rows, side=None, g34_nudge=0):
    return _init(rows, LDT, side, g34_nudge)


def f64_init(rows):
    return _init(rows, np.float64)


def init_refs(rows):
    """Every reference of init_state the thresholds (Gamma34 > 1, sigma) admit."""
    return [ref_init(rows, s) for s in ({}, {"g34": -1}, {"g34": 1}, {"sigma": -1}, {"sigma": 1})]


def init_U3_error(got, rows):
    """U3 against (Gamma34 - 1) m3 c^2 formed from the producer's own m3 and the stored Gamma34 the reference admits (rounded, +-2 ulps);
    0 against 0 where the state is not seeded."""
    got = np.asarray(got, dtype=np.float64)
    errs = []
    for k in (0, -1, 1, -2, 2):  # rel_Gamma in double is within 1.1 ulp of the exact value: two ulps of the rounded one
        r = ref_init(rows, {}, k)
        m3_ref = r[:, STATE.index("m3")]
        with np.errstate(all="ignore"):
            g34m1 = np.where(m3_ref != 0, r[:, STATE.index("U3")] / np.where(m3_ref != 0, m3_ref, 1), 0)
        errs.append(rel(got[:, STATE.index("U3")], g34m1 * ld(got[:, STATE.index("m3")])))
    return np.minimum.reduce(errs)


# ================================================================ the probe's input sets
_SETS = {}


def gclass(gm1):
    return np.where(np.asarray(gm1, dtype=np.float64) >= 1e-3, "g>=1e-3", "g<1e-3")


def sclass(sigma):
    s = np.asarray(sigma, dtype=np.float64)
    return np.where(s <= SIGMA_CUT * (1 - 1e-9), "hydro", np.where(s <= 10 * SIGMA_CUT, "near-cut", "magnetised"))


def _sigma_draw(rng, n):
    kind = rng.integers(0, 4, n)
    return np.where(kind == 0, 0.0, np.where(kind == 1, _logu(rng, SIGMA_CUT * (1 + 1e-9), 10 * SIGMA_CUT, n), _logu(rng, 1e-6, 1e3, n)))


def _set_rel_gamma(rng):
    g1 = 1 + _logu(rng, 1e-3, 1e3, N_RANDOM)
    g2 = np.maximum(1.0, 1 + (g1 - 1) * (1 - _logu(rng, 1e-12, 1.0, N_RANDOM)))
    e1 = 1 + _logu(rng, 1e-3, 1e3, 64)
    edge = np.concatenate([np.stack([e1, e1], 1), np.stack([e1, np.ones(64)], 1), np.stack([e1, e1 * (1 - 1e-12)], 1), [[1.0, 1.0]]])
    rows = np.concatenate([np.stack([g1, g2], 1), edge])
    kind = np.concatenate([np.full(N_RANDOM, "random"), np.full(edge.shape[0], "edge")])
    return rows, kind


def _set_shock_jump(rng):
    g = 1 + _logu(rng, 1e-15, 1e3, N_RANDOM)
    s = _sigma_draw(rng, N_RANDOM)
    ge = 1 + np.geomspace(1e-15, 1e3, 32)
    placed = np.concatenate([np.stack([ge, np.full(32, float(nudge(SIGMA_CUT, k)))], 1) for k in (-2, -1, 0, 1, 2)])
    edge = np.array([[1.0, 0.0], [1.0, 1e-7]])
    rows = np.concatenate([np.stack([g, s], 1), placed, edge])
    kind = np.concatenate([np.full(N_RANDOM, "random"), np.full(placed.shape[0], "placed"), np.full(edge.shape[0], "edge")])
    return rows, kind


def _set_sound_speed(rng):
    G = np.concatenate([1 + _logu(rng, 1e-15, 1e3, N_RANDOM), [1.0, float(nudge(1.0, 1))]])
    return G[:, None], np.concatenate([np.full(N_RANDOM, "random"), np.full(2, "edge")])


def _rvs_rows(rng, n):
    G4 = 1 + _logu(rng, 3.0, 1e3, n)
    G = np.maximum(1.0, G4 / (1 + _logu(rng, 1e-8, 1.0, n)))
    r, x4, m4 = _logu(rng, 1e-3, 1e6, n), _logu(rng, 1e-6, 1e2, n), _logu(rng, 1e-12, 1e-2, n)
    x3 = x4 * _logu(rng, 1e-8, 1.0, n)
    m3 = m4 * _logu(rng, 1e-8, 1.0, n)
    U3 = m3 * _logu(rng, 1e-9, 1e2, n)
    eps4 = G4 * m4 * (1 + _sigma_draw(rng, n))
    V3 = r * r * x3
    return np.stack([G, x4, x3, m3, U3, r, eps4, m4, G4, _logu(rng, 1e-6, 0.5, n), rng.integers(0, 2, n).astype(float),
                     V3 * _logu(rng, 1e-4, 1.0, n), _logu(rng, 1e-20, 1e-5, n), np.where(rng.integers(0, 2, n) == 0, 0.0, _logu(rng, 1e-12, 1e-2, n))], 1)


def _set_rvs_state(rng):
    rows = _rvs_rows(rng, N_RANDOM)
    i = {n: k for k, n in enumerate(RVS_IN)}
    # Gamma_th on GAMMA_CUT at -2 ... 2 ulps (of 1), crossing and after; sigma of the state on SIGMA_CUT at -2 ... 2 ulps (of 1 + sigma)
    base = _rvs_rows(rng, 16)
    placed = []
    for k in (-2, -1, 0, 1, 2):
        for flag in (0.0, 1.0):
            b = base.copy()
            b[:, i["U3"]] = b[:, i["m3"]] * (float(nudge(GAMMA_CUT, k)) - 1)
            b[:, i["crossing"]] = flag
            placed.append(b)
        b = base.copy()
        b[:, i["eps4"]] = b[:, i["Gamma4"]] * b[:, i["m4"]] * float(nudge(1 + SIGMA_CUT, k))
        b[:, i["crossing"]] = 1.0
        placed.append(b)
    placed = np.concatenate(placed)
    edge = _rvs_rows(rng, 8)  # an unshocked shell: m3 = 0 gives Gamma_th = 1, N_p = 0
    edge[:, i["m3"]] = 0.0
    edge[:, i["U3"]] = 0.0
    edge[:, i["crossing"]] = [0, 1] * 4
    out = np.concatenate([rows, placed, edge])
    kind = np.concatenate([np.full(N_RANDOM, "random"), np.full(placed.shape[0], "placed"), np.full(8, "edge")])
    return out, kind


def rvs_classes(rows):
    """(gamma class, sigma class) of VAG_MATH_RVS_STATE rows, from the reference's Gamma34 and sigma."""
    a = _cols(np.asarray(rows, dtype=np.float64), RVS_IN)
    g34 = ref_rel_Gamma(a["Gamma4"], a["Gamma"])
    sigma = (ld(a["eps4"]) / (ld(a["Gamma4"]) * ld(a["m4"])) - 1).astype(np.float64)
    return gclass((g34 - 1).astype(np.float64)), sclass(sigma)


def lattice_set():
    """[(ts, t_end, t_dec, T0, t_num, base_t_num)]: t_num 4 ... 64, both `plain` causes, n_post clamped at 2 and at t_num / 2."""
    rng = np.random.default_rng([SEED, 5])
    lats = []
    for t_num in (4, 5, 7, 8, 16, 24, 33, 48, 63, 64):
        ts, t_end = float(_logu(rng, 1e-4, 1e-1, 1)[0]), float(_logu(rng, 1e3, 1e6, 1)[0])
        for T0, t_dec, base in (
                (ts * 3.0, ts * 0.5, t_num),                 # refined, n_post from the ratio of the logarithms
                (ts * 0.5, ts * 40.0, max(2, t_num // 2)),   # t_dec decides t_refine
                (t_end / 15.0, ts, t_num),                   # t_refine just under t_end: n_post clamped at 2
                (ts * 1.5, ts, 4 * t_num),                   # base_t_num large: n_post >= t_num, clamped at t_num / 2
                (ts / 20.0, ts / 30.0, t_num),               # plain: t_refine <= ts
                (t_end, ts, t_num)):                       # plain: t_refine >= t_end
            lats.append((ts, t_end, float(t_dec), float(T0), t_num, base))
        # 10 T0 == ts and 10 T0 == t_end as the double product gives them: `<=` and `>=` make both plain
        lats.append((10 * (ts / 10.0), t_end, ts / 50.0, ts / 10.0, t_num, t_num))
        lats.append((ts, 10 * (t_end / 10.0), ts, t_end / 10.0, t_num, t_num))
    return lats


def lattice_rows(lats):
    """VAG_MATH_CROSS_LATTICE rows of every node of every lattice, and the lattice each row belongs to."""
    rows = np.array([list(lat) + [k] for lat in lats for k in range(lat[4])], dtype=np.float64)
    owner = np.concatenate([np.full(lat[4], j) for j, lat in enumerate(lats)])
    return rows, owner


def _set_extrap(rng):
    """Rows of 16 nodes: Gamma_th = 1 up to idx_cut, rising after; idx_cut 0 ... 16, inj above and at or below idx_cut."""
    rows, kind = [], []
    for rep in range(12):
        for c in range(0, EXT_NODES + 1):
            for inj in sorted({EXT_NODES, c + 1, c, max(c - 1, 0), 1}):
                if inj > EXT_NODES:
                    continue
                r = np.cumprod(1 + _logu(rng, 1e-2, 3.0, EXT_NODES)) * float(_logu(rng, 1e-3, 1e3, 1)[0])
                Gth = np.ones(EXT_NODES)
                Gth[c:] = 1 + np.sort(_logu(rng, 2e-6, 1e2, EXT_NODES - c))
                if c and rep % 4 == 1:
                    Gth[:c] = rng.choice([1.0, GAMMA_CUT, 1 + 5e-7], c)  # at and under the cut: not above it
                if c < EXT_NODES and rep % 4 == 2:
                    Gth[c] = float(nudge(GAMMA_CUT, 1))
                B = np.cumprod(_logu(rng, 0.5, 3.0, EXT_NODES)) * float(_logu(rng, 1e-6, 1e2, 1)[0])
                Np = np.cumprod(1 + _logu(rng, 1e-2, 3.0, EXT_NODES)) * float(_logu(rng, 1e30, 1e55, 1)[0])
                rows.append(np.concatenate([np.stack([r, Gth, B, Np], 1).ravel(), [inj]]))
                kind.append("idx_cut == 0" if c == 0 else "idx_cut >= nt - 2" if c >= EXT_NODES - 2 else "idx_cut >= inj" if c >= inj else "applies")
    return np.array(rows), np.array(kind)


def _set_pair_init(rng):
    n = 1024
    G4 = 1 + _logu(rng, 4.0, 1e3, n)
    T0 = _logu(rng, 2e-3, 2e1, n)
    deps = _logu(rng, 1e-8, 1e-1, n)
    dm = deps / (G4 * (1 + _sigma_draw(rng, n)))
    t0 = T0 * np.where(rng.integers(0, 2, n) == 0, _logu(rng, 1e-6, 0.99, n), _logu(rng, 1.01, 1e4, n))
    wind = rng.integers(0, 2, n).astype(float)
    rho = _logu(rng, 1e-21, 1e-15, n)
    A = np.where(wind != 0, _logu(rng, 1e-22, 1e-16, n), 0.0)
    r02 = np.where((wind != 0) & (rng.integers(0, 2, n) == 0), _logu(rng, 1e-6, 1e2, n), 0.0)
    rows = np.stack([G4, deps, dm, T0, t0, rng.choice([0.0, 0.1], n), wind, rho, A, r02], 1)
    early = rows[:64].copy()  # a start so early that the swept-up mass leaves Gamma34 == 1 exactly: the unseeded branch
    early[:, 4] = early[:, 3] * 1e-9
    early[:, 7] = 1e-24
    early[:, 8] = 0.0
    early[:, 6] = 0.0
    at = rows[64:96].copy()   # t0 == T0: the second form of x4
    at[:, 4] = at[:, 3]
    out = np.concatenate([rows, early, at])
    # a row is integrated only from Gamma > RS_GAMMA_LIMIT: where the swept-up mass would stop the shell at t0, thin the medium until
    # m2 / (dm0_dt T0) is drawn from [1e-8, 1] (m2 is linear in rho_ism and A)
    st = f64_init(out)
    heavy = st[:, STATE.index("Gamma")] < 2
    scale = np.where(heavy, _logu(rng, 1e-8, 1.0, out.shape[0]) * out[:, 2] * out[:, 3] / st[:, STATE.index("m2")], 1.0)
    out[:, 7] *= scale
    out[:, 8] *= scale
    return out, np.concatenate([np.full(n, "random"), np.full(64, "early"), np.full(32, "t0 == T0")])


_MAKERS = {"rel_gamma": (_set_rel_gamma, 1), "shock_jump": (_set_shock_jump, 2), "sound_speed": (_set_sound_speed, 3),
           "rvs_state": (_set_rvs_state, 4), "rvs_extrap": (_set_extrap, 6), "pair_init": (_set_pair_init, 7)}


def probe_set(name):
    """(rows [n][n_in], kind [n]) of a probe routine; "cross_lattice": (rows, the lattice of each row), with lattice_set().  One fixed
    seed; cached."""
    if name not in _SETS:
        if name == "cross_lattice":
            _SETS[name] = lattice_rows(lattice_set())
        else:
            make, k = _MAKERS[name]
            _SETS[name] = make(np.random.default_rng([SEED, k]))
    return _SETS[name]


def worst_by(err, *classes):
    """{class tuple: max error} of err [n] under the per-point class labels."""
    keys = np.array(["|".join(t) for t in zip(*classes)]) if classes else np.full(np.shape(err), "")
    return {tuple(k.split("|")) if classes else (): float(np.max(err[keys == k])) for k in np.unique(keys)}


# ================================================================ a producer's outputs against the reference
def point_errors(name, out):
    """A producer's outputs `out` [n][n_out] (the float64 restatement's or the device's) on probe_set(name), each value against the nearest
    reference the thresholds admit: {quantity: (relative error [m], class key [m] -- the tuple a ceiling is looked up with, joined with
    ";" -- and the rows [m] compared)}.  A quantity in bars is |fast - exact| of the producer's own two columns.  `counts` holds what must
    be zero: points where jump_4vel_f is not jump_4vel's bits although sigma > SIGMA_CUT, early-return rows the extrapolation changed."""
    rows, kind = probe_set(name)
    out = np.asarray(out, dtype=np.float64)
    n = rows.shape[0]
    every = np.arange(n)
    res, counts = {}, {}

    def put(q, err, classes=(), idx=every):
        key = np.array([";".join((q,) + t) for t in zip(*classes)]) if classes else np.full(np.shape(err), q)
        res[q] = (np.asarray(err, dtype=np.float64), key, idx)

    if name == "rel_gamma":
        refs = list(admitted(lambda s: ref_rel_Gamma(rows[:, 0], rows[:, 1], s), ("denom",)))
        put("rel_Gamma", nearest(out[:, 0], refs))
        put("|rel_Gamma_f - rel_Gamma|", rel(out[:, 1], ld(out[:, 0])))
    elif name == "shock_jump":
        g, s = rows[:, 0], rows[:, 1]
        gc, sc = gclass(g - 1), sclass(s)
        put("u_down", rel(out[:, 0], ref_downstr_4vel(g, s)), (gc, sc))
        put("jump", rel(out[:, 1], ref_jump_4vel(g, s)), (gc, sc))
        hyd = s <= SIGMA_CUT
        put("|jump_f - jump|", rel(out[hyd, 2], ld(out[hyd, 1])), (gc[hyd],), every[hyd])
        counts["jump_4vel_f is not jump_4vel where sigma > SIGMA_CUT"] = int(np.sum(out[~hyd, 2] != out[~hyd, 1]))
    elif name == "sound_speed":
        put("sound_speed", rel(out[:, 0], ref_sound_speed(rows[:, 0])))
        put("|sound_speed_f - sound_speed|", rel(out[:, 1], ld(out[:, 0])))
    elif name == "rvs_state":
        refs = list(admitted(lambda s: ref_rvs_state(rows, s, out[:, 0]), ("sigma", "gth")))
        gc, sc = rvs_classes(rows)
        for j, q in enumerate(RVS_OUT):
            put("rvs." + q, nearest(out[:, j], [r[:, j] for r in refs]), (gc, sc) if q in ("B", "rho3", "B3_ordered") else ())
    elif name == "rvs_extrap":
        ref, applies = ref_extrap(rows)
        got = out.reshape(-1, EXT_NODES, 3)
        for j, q in enumerate(("Gamma_th", "B", "N_p")):
            put("extrap." + q, rel(got[applies, :, j], ref[applies, :, j]).max(axis=1), (), every[applies])
        given = rows[:, :4 * EXT_NODES].reshape(-1, EXT_NODES, 4)[:, :, 1:]
        counts["rows of an early return that the extrapolation changed"] = int(np.sum(np.any(got[~applies] != given[~applies], axis=(1, 2))))
    elif name == "pair_init":
        refs = init_refs(rows)
        sc = sclass(rows[:, 1] / (rows[:, 0] * rows[:, 2]) - 1)
        for j, q in enumerate(STATE):
            e = init_U3_error(out, rows) if q == "U3" else nearest(out[:, j], [r[:, j] for r in refs])
            put("init." + q, e, (sc,) if q in ("m3", "U3") else ())
    else:
        raise KeyError(name)
    return res, counts


def errors(name, out):
    """{(quantity, class ...): max relative error} of point_errors, and its counts."""
    pe, counts = point_errors(name, out)
    res = {}
    for err, key, _ in pe.values():
        for k in np.unique(key):
            res[tuple(k.split(";"))] = float(err[key == k].max())
    return res, counts


def lattice_errors(lats, produced):
    """produced[j]: dict(n_pre, n_post, plain, nodes [t_num]) of lattice j.  -> (max relative node error against the nearest admitted
    reference with the producer's integers, problems: the lattices whose integers no reference admits or whose nodes do not ascend)."""
    worst, problems = 0.0, []
    for j, (lat, got) in enumerate(zip(lats, produced)):
        same = [v for v in lattice_variants(lat) if (v["n_pre"], v["n_post"], v["plain"]) == (int(got["n_pre"]), int(got["n_post"]), int(got["plain"]))]
        nodes = np.asarray(got["nodes"], dtype=np.float64)
        if not same:
            problems.append(f"lattice {j} {lat}: n_pre, n_post, plain = {got['n_pre']}, {got['n_post']}, {got['plain']}: no reference admits them")
            continue
        if not np.all(np.diff(nodes) > 0):
            problems.append(f"lattice {j} {lat}: the nodes do not strictly ascend")
        worst = max(worst, min(float(rel(nodes, v["nodes"]).max()) for v in same))
    return worst, problems


# ================================================================ ceilings: 25 x the float64 figure beside each (CPU_FIGURES, measured by
# tests/test_reverse_state_host.py on the restatements above with numpy on glibc; that test asserts them again)
CEILING_FACTOR = 25
_G, _S = ("g<1e-3", "g>=1e-3"), ("hydro", "near-cut", "magnetised")


def _by_class(q, table):
    """table[g class][sigma class] -> {(q, g, s): figure}"""
    return {(q, g, s): f for g, row in zip(_G, table) for s, f in zip(_S, row)}


# The maxima of the float64 restatements over the probe sets, rounded up to two digits.  Classes: gamma_rel - 1 (Gamma34 - 1 for the cell
# state) below 1e-3 or not; sigma <= SIGMA_CUT ("hydro"), within a decade above it ("near-cut"), beyond ("magnetised").  The large
# figures are the condition of the formula, not of its evaluation: with gamma_rel - 1 << sigma the jump is 1 + O(sqrt((gamma_rel - 1) /
# sigma)), and the cell state and init_state form gamma_rel = 1 + d^2 / denom and sigma = eps4 / (Gamma4 m4 c^2) - 1 as doubles first,
# which leaves gamma_rel - 1 and sigma with an absolute error of 1e-16: any double implementation is that far from the reference.
CPU_FIGURES = {
    ("rel_Gamma",): 2.5e-16, ("sound_speed",): 4.1e-16,
    #                      hydro    near-cut  magnetised
    **_by_class("u_down", ((5.0e-16, 3.0e-10, 4.6e-09),      # gamma_rel - 1 < 1e-3
                           (8.3e-16, 8.0e-16, 1.3e-14))),    # gamma_rel - 1 >= 1e-3
    **_by_class("jump",   ((4.5e-16, 3.7e-11, 4.3e-12),
                           (5.3e-16, 6.2e-16, 9.0e-15))),
    ("rvs.Gamma_th",): 2.2e-16, ("rvs.N_p",): 1.2e-16, ("rvs.V3_comv",): 2.2e-16,
    **_by_class("rvs.B",          ((3.6e-16, 1.4e-05, 9.1e-07),
                                   (3.4e-16, 4.6e-11, 2.7e-12))),
    **_by_class("rvs.rho3",       ((7.0e-16, 1.4e-05, 2.0e-06),
                                   (5.9e-16, 1.3e-13, 8.4e-14))),
    **_by_class("rvs.B3_ordered", ((0.0,     1.4e-05, 2.0e-06),   # (sigma <= SIGMA_CUT: no ordered field, exactly)
                                   (0.0,     8.6e-11, 4.7e-12))),
    ("lattice.node",): 4.7e-15,
    ("extrap.Gamma_th",): 1.2e-16, ("extrap.B",): 1.4e-12, ("extrap.N_p",): 4.0e-12,   # 2^(slope x log2 ratio) of values up to 2^180
    ("init.Gamma",): 3.1e-15, ("init.x4",): 4.9e-16, ("init.x3",): 4.9e-16, ("init.m2",): 5.7e-15, ("init.U2",): 7.6e-15,
    ("init.r",): 5.4e-16, ("init.t_comv",): 4.4e-16, ("init.eps4",): 1.1e-16, ("init.m4",): 1.2e-16,
    ("init.m3", "hydro"): 2.2e-15, ("init.m3", "near-cut"): 2.2e-06, ("init.m3", "magnetised"): 4.2e-07,
    ("init.U3", "hydro"): 1.8e-15, ("init.U3", "near-cut"): 4.2e-15, ("init.U3", "magnetised"): 3.1e-15,
}
# |fast - exact| / |exact|: the maxima over the probe sets and over every sign pattern of the perturbed reciprocals and square roots
# (fast_bound), rounded up to two digits.  These are bounds, not measurements: they are the ceilings of the differences as they stand.
FAST_BOUNDS = {
    ("|rel_Gamma_f - rel_Gamma|",): 3.9e-15, ("|sound_speed_f - sound_speed|",): 6.8e-15,
    ("|jump_f - jump|", "g<1e-3"): 1.1e-14, ("|jump_f - jump|", "g>=1e-3"): 1.1e-14,
}


def ceiling(quantity, *cls):
    key = (quantity,) + tuple(cls)
    return FAST_BOUNDS[key] if key in FAST_BOUNDS else CEILING_FACTOR * CPU_FIGURES[key]


def key_ceilings(keys):
    """The ceiling of every per-point class key of point_errors."""
    return np.array([ceiling(*k.split(";")) for k in keys])
