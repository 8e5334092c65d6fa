"""Extended-precision reference of the inverse-Compton routines below vag_ic_photon_kernel (tests/test_ic_state_host.py,
tests/test_ic_state.py).  Device: vag_ic.h and vag_ic_kernels.h -- the Klein-Nishina table the context builds on the host and its two
look-ups (compton_correction_pair_lg2, _pair_node), ic_table_eval_hdr, power_law_bin_integral, suffix_scan4 and electron_column_den,
IcY, one pass of the gamma_c and gamma_M fixed points, the loops themselves (held by a property: the result is a stopping iterate the
rule admits for the reference's own iteration from the same start), syn_gamma_a_ic and determine_regime, each through its probe routine
(vag_debug_device_math).  vag_ic_photon_kernel's body and the plan and band kernels are NOT here: they stay held end to end
(tests/test_gpu_parity.py::test_ssc_*, tests/test_ic_diagonal_identity.py).

Every routine is restated twice, as tests/_rsref.py does:
* `ref_*`: the formula in numpy.longdouble on the float64 inputs taken exactly (inverse-compton.cpp:257-283 for the cross-section
  ratio, :285-343 for the table, :356-385 for the look-up; synchrotron.cpp:261-309 for the column density); the Klein-Nishina ratio
  itself in mpmath at KN_DPS digits, because the float64 formula cancels in its middle branch;
* `f64_*`: the same in float64 in the device's statement order -- what IEEE double with the C library gives, the figure the ceilings
  come from -- carrying the deliberate defects of the sensitivity checks (`mut`).

The look-up's reference is the SAME linear interpolation in long double on the exact nodes: what linear interpolation on 128 nodes costs
against the exact function (4e-4) is the upstream table's design and is printed by the host test, not gated.  Likewise the low tail's
logarithm -(2x + 2x^2) log2(e) is the closed form the device states, two terms of log2(1 - 2x).

Thresholds.  A comparison of a COMPUTED value with a threshold (lg2_nu + log2(h / m_e c^2) against the table's ends, a node's x against
1e-2 and 1e2, |s1| against 1e-3, x against the `last` the probe forms from first and n) is decided exactly and, where the value is
within two roundings of the threshold, both ways: the device is compared with the NEAREST admitted reference and is never excused.  A
comparison of an INPUT double with a threshold (lg2_x handed to the node form, gamma <= gamma_c, x against first, th_min, th_max, f > 0)
involves no rounding and is decided exactly.

Everything is in the engine's code units (_mathref's constants)."""
import math

import numpy as np

import _elecref as er
import _mathref as mr
from _rsref import LDT, NEAR, _logu, _mp, ld, nearest, nudge, rel

mpmath = mr.mpmath
SEED = 20261021
N_RANDOM = 4096
KN_DPS = 50
KN_LUT_N = 128
KN_LG2_XMIN, KN_LG2_XMAX = -6.6438561897747247, 6.6438561897747247
KN_STEP = (KN_LG2_XMAX - KN_LG2_XMIN) / (KN_LUT_N - 1)
KN_INV_STEP = 1.0 / KN_STEP
C_H = 6.63e-27 * er.U_ERG * mr.U_SEC
X_PER_NU = C_H / (mr.C_ME * mr.C_C2)  # x = h nu / (m_e c^2), the double the device's constant is the logarithm of
LG2_X_PER_NU = float(np.log2(X_PER_NU))
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LN2_LD = np.log(LDT(2))
IC_Q = 3.321928094887362 / 8
IC_INV_STEP = 1.0 / (2 * IC_Q)
TAB_WORDS = 16
E_RCP_ESTIMATE = 4.6e-8  # the hardware reciprocal estimate before its Newton steps (vag_device.h)

MUTATIONS = ("low_tail_first_order_log", "first_order_ln2x", "high_tail_without_half", "idx_not_clamped", "frac_before_clamp",
             "breach_ignores_theoretical_range", "rcp_without_newton", "series_branch_at_any_s1", "scan_drops_lane63",
             "ic_factor_below_gamma_c", "regime_sets_swapped", "mid_slope_p_minus_2", "gamma_c_without_plus_4", "segment_1_at_a_tie",
             "gamma_a_without_ic_factor", "gamma_a_without_plus_1")


# ================================================================ the Klein-Nishina ratio and its table
def kn_ratio_mp(x, branch=None):
    """sigma / sigma_T at x = h nu / (m_e c^2) as compton_ratio_from_x defines it (inverse-compton.cpp:257-283): 1 - 2x below 1e-2, the
    asymptotic form above 1e2, the Klein-Nishina formula between.  `branch` (-1 / 0 / +1) overrides the choice."""
    x = mpmath.mpf(x)
    if branch is None:
        branch = -1 if x < mpmath.mpf(1e-2) else (1 if x > mpmath.mpf(1e2) else 0)
    if branch < 0:
        return 1 - 2 * x
    if branch > 0:
        return mpmath.mpf(3) / 8 * (mpmath.log(2 * x) + mpmath.mpf(1) / 2) / x
    l = mpmath.log(1 + 2 * x)
    return mpmath.mpf(3) / 4 * ((1 + x) / x ** 3 * (2 * x * (1 + x) / (1 + 2 * x) - l) + l / (2 * x) - (1 + 3 * x) / (1 + 2 * x) ** 2)


def _to_ld(v):
    hi = float(v)
    return LDT(hi) + LDT(float(v - mpmath.mpf(hi)))


_NODES = {}


def kn_node_lg2x(k):
    """log2 x of node k as the host loop forms it (a double)."""
    return KN_LG2_XMIN + KN_STEP * np.asarray(k, dtype=np.float64)


def kn_nodes(branch_ends=(None, None)):
    """(ratio [128], log2 ratio [128]) in long double: the exact ratio at x = 2^(the node's double log2 x).  `branch_ends`: the branch
    forced at node 0 and at node 127, which sit on the thresholds 1e-2 and 1e2 to within the rounding of exp2."""
    if branch_ends not in _NODES:
        r, lr = np.zeros(KN_LUT_N, dtype=LDT), np.zeros(KN_LUT_N, dtype=LDT)
        with mpmath.workdps(KN_DPS):
            for k in range(KN_LUT_N):
                x = mpmath.power(2, mpmath.mpf(float(kn_node_lg2x(k))))
                b = branch_ends[0] if k == 0 else (branch_ends[1] if k == KN_LUT_N - 1 else None)
                v = kn_ratio_mp(x, b)
                r[k], lr[k] = _to_ld(v), _to_ld(mpmath.log(v, 2))
        _NODES[branch_ends] = (r, lr)
    return _NODES[branch_ends]


def kn_end_branches():
    """The branches node 0 and node 127 may take: the exact one, and the other where 2^(log2 x) is within two roundings of the threshold."""
    res = []
    with mpmath.workdps(KN_DPS):
        for k, thr, far in ((0, 1e-2, -1), (KN_LUT_N - 1, 1e2, 1)):
            x = mpmath.power(2, mpmath.mpf(float(kn_node_lg2x(k))))
            near = abs(x - mpmath.mpf(thr)) <= 2 * 2.0 ** -52 * thr
            res.append((None, 0, far) if near else (None,))
    return res


def f64_kn_lut(k, mut=()):
    """The host loop of vag_ctx_create in float64."""
    x = np.exp2(kn_node_lg2x(k))
    with np.errstate(all="ignore"):
        lo = 1 - 2 * x
        hi = 3. / 8 * (np.log(2 * x) + 0.5) / x
        l = np.log1p(2.0 * x)
        invx = 1.0 / x
        invx2 = invx * invx
        invt1 = 1.0 / (1.0 + 2.0 * x)
        mid = 0.75 * ((1.0 + x) * invx2 * invx * (2.0 * x * (1.0 + x) * invt1 - l) + 0.5 * l * invx - (1.0 + 3.0 * x) * (invt1 * invt1))
    ratio = np.where(x < 1e-2, lo, np.where(x > 1e2, hi, mid))
    return np.stack([ratio, np.log2(ratio)], axis=1)


def ref_kn_lut_all():
    """Every admitted table: [(ratio, log2 ratio)] over the branches the two end nodes may take."""
    b0, b1 = kn_end_branches()
    return [kn_nodes((a, b)) for a in b0 for b in b1]


def _interp(T, lg2_x, nodes):
    """Linear interpolation in log2 x on the table (inverse-compton.cpp:356-385): (corr, lg2_corr) in arithmetic T."""
    pos = np.minimum(np.maximum((lg2_x - T(KN_LG2_XMIN)) * T(KN_INV_STEP), T(0)), T(KN_LUT_N - 1))
    # (the clamp at N - 2 is never the deciding one: (lg2_x - XMIN) * inv_step stays below 127 for every double lg2_x < XMAX -- one step
    # below XMAX it is 127 - 8.5e-15, more than half a spacing of doubles there -- so an unclamped index is not a defect a value can show)
    idx = np.clip(np.floor(pos).astype(np.float64), 0, KN_LUT_N - 2).astype(int)
    frac = pos - idx.astype(T)
    r, lr = (np.asarray(a, dtype=T) for a in nodes)
    return r[idx] + (r[idx + 1] - r[idx]) * frac, lr[idx] + (lr[idx + 1] - lr[idx]) * frac


def _kn_pair(T, lg2_x, x, nodes, side_lo, side_hi, mut=()):
    """(corr, lg2_corr) of compton_correction_pair at log2 x (with x = 2^lg2_x given) in arithmetic T.  side_lo / side_hi [n] of
    {-1, +1, 0}: how lg2_x > XMIN and lg2_x >= XMAX are decided (0: exactly)."""
    below = np.where(side_lo == 0, ~(lg2_x > T(KN_LG2_XMIN)), side_lo < 0)
    above = np.where(side_hi == 0, lg2_x >= T(KN_LG2_XMAX), side_hi > 0)
    with np.errstate(all="ignore"):
        c_lo = 1 - 2 * x
        l_lo = -(2 * x if "low_tail_first_order_log" in mut else 2 * x + 2 * x * x) * T(LOG2E if T is np.float64 else 1 / LN2_LD)
        ln2 = T(LN2) if T is np.float64 else LN2_LD
        a = T(0.375) * (((lg2_x + 1.0) * ln2 if "first_order_ln2x" not in mut else lg2_x * ln2) + T(0.0 if "high_tail_without_half" in mut else 0.5))
        inv = 1 / np.where(x > 0, x, 1)
        c_hi, l_hi = a * inv, np.log2(np.where(a > 0, a, 1)) - lg2_x
        c_in, l_in = _interp(T, lg2_x, nodes)
    corr = np.where(below, np.where(x > 0, c_lo, 0), np.where(above, c_hi, c_in))
    lg = np.where(below, np.where(x > 0, l_lo, -np.inf), np.where(above, l_hi, l_in))
    return corr, lg


def _kn_lg2x(rows):
    """The argument of the node form: column 1, or where it is NaN what the first form makes of column 0 (a double sum)."""
    return np.where(np.isnan(rows[:, 1]), rows[:, 0] + LG2_X_PER_NU, rows[:, 1])


def f64_kn_corr(rows, mut=()):
    nodes = tuple(f64_kn_lut(np.arange(KN_LUT_N)).T)
    z = np.zeros(rows.shape[0], dtype=int)
    with np.errstate(all="ignore"):
        lx = rows[:, 0] + LG2_X_PER_NU
        a = _kn_pair(np.float64, lx, np.exp2(lx), nodes, z, z, mut)
        lx = _kn_lg2x(rows)
        b = _kn_pair(np.float64, lx, np.exp2(lx), nodes, z, z, mut)
    return np.stack([a[0], a[1], b[0], b[1]], axis=1)


def ref_kn_corr(rows):
    """[out [n][4] in long double] over everything the thresholds admit: the tables of ref_kn_lut_all and, for the first form, both sides
    of the table's ends where lg2_nu + log2(h / m_e c^2) is within two roundings of them.  The node form's lg2_x is an input."""
    with np.errstate(all="ignore"):
        lx1 = ld(rows[:, 0]) + np.log2(LDT(X_PER_NU))
    scale = np.abs(rows[:, 0]) + abs(LG2_X_PER_NU)
    near_lo = np.abs((lx1 - LDT(KN_LG2_XMIN)).astype(np.float64)) <= 2 * NEAR * scale
    near_hi = np.abs((lx1 - LDT(KN_LG2_XMAX)).astype(np.float64)) <= 2 * NEAR * scale
    # the node form: lg2_x as given, decided exactly; a NaN stands for the first form's own sum and is referred to as that form is
    own = np.isnan(rows[:, 1])
    l2 = ld(np.where(own, 0.0, rows[:, 1]))
    z = np.zeros(rows.shape[0], dtype=int)
    res = []
    for nodes in ref_kn_lut_all():
        with np.errstate(all="ignore"):
            b = _kn_pair(LDT, l2, np.exp2(l2), nodes, z, z)
        for s in (0, -1, 1):
            with np.errstate(all="ignore"):
                a = _kn_pair(LDT, lx1, np.exp2(lx1), nodes, np.where(near_lo, s, 0), np.where(near_hi, s, 0))
            res.append(np.stack([a[0], a[1], np.where(own, a[0], b[0]), np.where(own, a[1], b[1])], axis=1))
    return res


def kn_class(lg2_x):
    return np.where(~(lg2_x > KN_LG2_XMIN), "below", np.where(lg2_x >= KN_LG2_XMAX, "above", "table"))


# ================================================================ ic_table_eval_hdr
def tab_last(first, n, fused):
    """`last` as the probe forms it, ic_out_node(first, 0, n - 1) = first + IC_Q (0 + 2 (n - 1)): the sum rounded after the product
    (fused False) or the product kept exact (one fma)."""
    first, n = np.asarray(first, dtype=np.float64), np.asarray(n, dtype=np.float64)
    if fused:
        return (ld(first) + LDT(IC_Q) * ld(2.0 * (n - 1))).astype(np.float64)  # (the product of a double and a small integer is exact in 64 bits)
    return first + IC_Q * (0.0 + 2.0 * (n - 1))


def _table(T, rows, last, mut=()):
    n, first, th_min, th_max, x = (rows[:, j] for j in range(5))
    words = rows[:, 5:]
    empty, above = n < 2, x > last
    inside = ((x < th_max) | ("breach_ignores_theoretical_range" in mut), (x > th_min) | ("breach_ignores_theoretical_range" in mut))
    breach = (~empty & ((above & inside[0]) | ((x < first) & inside[1]))).astype(int) | np.where(n < 0, 4, 0)
    with np.errstate(all="ignore"):
        u = (x.astype(T) - first.astype(T)) * T(IC_INV_STEP)
        raw = np.floor(u)
        fl = raw if "idx_not_clamped" in mut else np.minimum(np.maximum(raw, 0), np.maximum(n - 2.0, 0).astype(T))
        frac = u - (raw if "frac_before_clamp" in mut else fl)
        idx = np.clip(fl.astype(np.float64), 0, TAB_WORDS - 2).astype(int)  # (only a defect reaches past the words; NaN stands there)
        i = np.arange(rows.shape[0])
        lo, hi = words[i, idx].astype(T), words[i, idx + 1].astype(T)
        val = lo + frac * (hi - lo)
    return np.where(empty | above, -np.inf, val), breach


def f64_table(rows, mut=()):
    v, b = _table(np.float64, rows, tab_last(rows[:, 1], rows[:, 0], False), mut)
    return np.stack([v, b.astype(np.float64)], axis=1)


def ref_table(rows):
    """[(value in long double, breach)] for each `last` the probe may have formed."""
    return [_table(LDT, rows, tab_last(rows[:, 1], rows[:, 0], f)) for f in (False, True)]


# ================================================================ power_law_bin_integral
def _bin(T, rows, side, mut=()):
    f_lo, f_hi, nu_lo, nu_hi, l_lo, l_hi, lg2r, inv, trap = (rows[:, j].astype(T) for j in range(9))
    with np.errstate(all="ignore"):
        s1 = 1 + (l_hi - l_lo) * inv
        big = np.abs(s1) > T(1e-3)
        if side is not None:
            # (with lg2f_lo = 0 and inv_lg2r = 1 nothing rounds on the way to s1: those rows are decided exactly)
            rounds = (rows[:, 4] != 0) | (rows[:, 7] != 1)
            near = rounds & (np.abs((np.abs(s1) - T(1e-3)).astype(np.float64)) <= 2 * NEAR * (1 + np.abs(((l_hi - l_lo) * inv).astype(np.float64))))
            big = np.where(near, side > 0, big)
        if "series_branch_at_any_s1" in mut:
            big = np.zeros_like(big)
        r = 1 / np.where(s1 == 0, 1, s1)
        if "rcp_without_newton" in mut:
            r = r * (1 + E_RCP_ESTIMATE)
        main = (f_hi * nu_hi - f_lo * nu_lo) * r
        series = f_lo * nu_lo * lg2r * (T(LN2) if T is np.float64 else LN2_LD)
    out = np.where(big, main, series)
    return np.where(~(rows[:, 0] > 0) | ~(rows[:, 1] > 0), trap, out), s1


def f64_bin(rows, mut=()):
    return _bin(np.float64, rows, None, mut)[0][:, None]


def ref_bin(rows):
    return [_bin(LDT, rows, s)[0] for s in (None, -1, 1)]


def bin_class(rows):
    """`trap`, `series` (|s1| <= 1e-3), `s1~1e-3` (within 1e-12 of the threshold: either branch, and the main one at its worst), or the
    decade of |s1|: the numerator f_hi nu_hi - f_lo nu_lo of a power law cancels as 1 / |s1|."""
    s1 = np.abs(_bin(LDT, rows, None)[1].astype(np.float64))
    c = np.where(s1 <= 1e-3, "series", np.where(s1 < 1e-2, "s1<1e-2", np.where(s1 < 1e-1, "s1<1e-1", "s1>=1e-1")))
    c = np.where(np.abs(s1 - 1e-3) <= 1e-15, "s1~1e-3", c)
    return np.where(~(rows[:, 0] > 0) | ~(rows[:, 1] > 0), "trap", c)


# ================================================================ suffix_scan4
def f64_scan(rows, mut=()):
    """The wavefront's order of additions: four words per lane, a log-step scan over the lanes' totals, then each lane's own words."""
    w = rows.reshape(-1, 64, 4)
    a, b, c, d = (w[:, :, j] for j in range(4))
    S = (a + b) + (c + d)
    top = 63 if "scan_drops_lane63" in mut else 64
    off = 1
    while off < 64:
        t = np.concatenate([S[:, off:], np.zeros((S.shape[0], off))], axis=1)
        S = np.where(np.arange(64) + off < top, S + t, S)
        off <<= 1
    nxt = np.concatenate([S[:, 1:], np.zeros((S.shape[0], 1))], axis=1)
    c3 = nxt + d
    c2 = c3 + c
    c1 = c2 + b
    return np.stack([c1 + a, c1, c2, c3], axis=2).reshape(-1, 4)


def ref_scan(rows):
    """math.fsum of every suffix of each wavefront's 256 words."""
    w = rows.reshape(-1, 256)
    out = np.empty_like(w)
    for j, v in enumerate(w):
        v = v.tolist()
        out[j] = [math.fsum(v[d:]) for d in range(256)]
    return out.reshape(-1, 4)  # (correctly rounded: the error measured against it is at most half an ulp larger than the true one)


# ================================================================ electron_column_den
def _column(T, rows, mut=()):
    g, gm, gc, gM, p, regime, cd, Yc, Yg = (rows[:, j].astype(T) if j != 5 else rows[:, j] for j in range(9))
    sets = ((3, 4, 6), (1, 2, 5)) if "regime_sets_swapped" in mut else ((1, 2, 5), (3, 4, 6))
    slow, fast = np.isin(regime, sets[0]), np.isin(regime, sets[1])
    with np.errstate(all="ignore"):
        if T is np.float64:  # the device's statement order: exp and pow through exp2 / log2
            e1 = np.exp2((-g / gM - gm / g) * LOG2E)
            s_slow = (p - 1) / gm * e1 * np.exp2(-p * np.log2(g / gm)) * gc / (g + gc)
            e2 = np.exp2((-g / gM - gc / g) * LOG2E)
            s_fast = e2 * gc / (g * g) / (1.0 + np.exp2((p - 1) * np.log2(g / gm)))
        else:  # synchrotron.cpp:261-309
            s_slow = (p - 1) / gm * np.exp(-g / gM - gm / g) * (g / gm) ** (-p) * gc / (g + gc)
            s_fast = np.exp(-g / gM - gc / g) * gc / (g * g) / (1 + (g / gm) ** (p - 1))
        spec = np.where(slow, s_slow, np.where(fast, s_fast, 0))
        plain = cd * spec
        cooled = cd * spec * (1 + Yc) / (1 + Yg)
    return np.where((rows[:, 0] <= rows[:, 2]) & ("ic_factor_below_gamma_c" not in mut), plain, cooled)


def f64_column(rows, mut=()):
    return _column(np.float64, rows, mut)[:, None]


def ref_column(rows):
    return _column(LDT, rows)


def column_den_mp(row):
    with mpmath.workdps(KN_DPS):
        g, gm, gc, gM, p, regime, cd, Yc, Yg = (mpmath.mpf(float(v)) if np.isfinite(v) else mpmath.inf for v in row)
        r = int(row[5])
        if r in (1, 2, 5):
            spec = (p - 1) / gm * mpmath.exp(-g / gM - gm / g) * (g / gm) ** (-p) * gc / (g + gc)
        elif r in (3, 4, 6):
            spec = mpmath.exp(-g / gM - gc / g) * gc / (g * g) / (1 + (g / gm) ** (p - 1))
        else:
            return LDT(0)
        return _to_ld(cd * spec if row[0] <= row[2] else cd * spec * (1 + Yc) / (1 + Yg))


# ================================================================ IcY (inverse-compton.h:28-76, inverse-compton.cpp:18-187)
K_HAT = mr.C_ME * mr.C_C2 / C_H                             # gamma_hat nu of an electron whose photons sit at the Klein-Nishina limit
K_SYN_GAMMA = 4 * mr.C_PI * mr.C_ME * mr.C_C / (3 * mr.C_E)  # syn_gamma^2 B / nu
STOP = 1e-3                                                  # the relative step both fixed points stop on
ICY_OUT = ("gamma_m_hat", "gamma_c_hat", "gamma_self", "regime", "size", "s0", "l0", "c0", "s1", "l1", "c1", "s2", "l2", "c2",
           "Y(g0)", "Y(g1)", "Y(nu0)", "Y(nu1)")


class Icy:
    """Y(gamma) of a batch of cells in arithmetic T: log2 Y = c_i + s_i log2 gamma on segment i, the segments that
    InverseComptonY::build_segments makes for regimes 0 (Thomson: Y = Y_T), 1 (gamma_m < gamma_c) and 2.  Float64 follows the device's
    statement order (everything in log2, gamma_self = 2^((log2 gamma_m_hat + 2 log2 gamma_m) / 3)); long double follows the formulas:
    gamma_m_hat = max(m_e c^2 / (h nu_m), 1), gamma_self^3 = gamma_m_hat gamma_m^2, gamma_hat(g) = max(gamma_self^3 / g^2, 1).
    `side`: how the two max(.., 1) are decided where the argument is within 4 roundings of 1 (None: exactly)."""

    def __init__(self, T, gm, p, B, mut=()):
        self.T, self.mut = T, mut
        self.gm, self.p, self.B = gm.astype(T), p.astype(T), B.astype(T)
        with np.errstate(all="ignore"):
            nu_m = np.where(B == 0, 0, T(mr.K_SYN_FREQ) * self.B * self.gm * self.gm)
            self.m_raw = T(K_HAT) / nu_m
            self.lg2_gm = np.log2(self.gm)

    def _clamp(self, raw, side):
        one = raw <= 1
        if side is not None:
            one = np.where(np.abs((raw - 1).astype(np.float64)) <= 4 * NEAR, side < 0, one)
        return np.where(one, self.T(1), raw), one

    def build(self, gc, YT, kn, side=None):
        """The constructor's gamma_c part and update_cooling_breaks: kn [n] bool."""
        T = self.T
        gc, YT = gc.astype(T), YT.astype(T)
        with np.errstate(all="ignore"):
            self.gm_hat, m_one = self._clamp(self.m_raw, side)
            lm = np.where(m_one, T(0), np.log2(self.gm_hat))
            if T is np.float64:
                lg2_self = (lm + 2 * self.lg2_gm) * (1.0 / 3.0)
                self.self_ = np.exp2(lg2_self)
                self3 = self.self_ * self.self_ * self.self_
                c_raw = self3 * (1 / (gc * gc))
                lc_raw = 3 * lg2_self - 2 * np.log2(gc)
                self.gc_hat, c_one = self._clamp(c_raw, side)
                lc = np.where(lc_raw > 0, lc_raw, 0.0) if side is None else np.where(c_one, 0.0, lc_raw)
            else:
                self3 = self.gm_hat * self.gm * self.gm
                self.self_ = np.cbrt(self3)
                self.gc_hat, c_one = self._clamp(self3 / (gc * gc), side)
                lc = np.where(c_one, T(0), np.log2(self.gc_hat))
            self.regime = np.where(kn, np.where(self.gm < gc, 1, 2), 0)
            r1 = self.regime == 1
            mid = T(0.5) * (self.p - (T(2.0) if "mid_slope_p_minus_2" in self.mut else T(3.0)))
            self.size = np.where(kn, 3, 1)
            z = np.zeros(gc.shape, dtype=T)
            self.s = [z, np.where(r1, mid, T(-0.5)), z + (-T(4) / 3)]
            self.l = [z, np.where(r1, lc, lm), np.where(r1, lm, lc)]
            c0 = np.log2(YT)
            if T is np.float64:  # add_segment: the value at the new lower end, minus the new slope times it
                c1 = (c0 + self.s[0] * self.l[1]) - self.s[1] * self.l[1]
                c2 = (c1 + self.s[1] * self.l[2]) - self.s[2] * self.l[2]
            else:
                c1 = c0 - self.s[1] * self.l[1]
                c2 = c0 + self.s[1] * (self.l[2] - self.l[1]) - self.s[2] * self.l[2]
            self.c = [c0, c1, c2]
            # what the subtractions cancel from: the metric of the constants
            self.c_scale = [np.abs(c0), np.abs(c0) + np.abs(self.s[1] * self.l[1]),
                            np.abs(c0) + np.abs(self.s[1] * self.l[1]) + np.abs(self.s[1] * self.l[2]) + np.abs(self.s[2] * self.l[2])]
        return self

    def lg2_Y(self, lx):
        """log2 Y at log2 gamma = lx."""
        T = self.T
        with np.errstate(all="ignore"):
            if T is np.float64:
                top = (self.size > 2) & (lx >= self.l[2])
                mid = (self.size > 1) & (lx >= self.l[1])
                if "segment_1_at_a_tie" in self.mut:
                    top = top & (self.l[2] > self.l[1])
                return np.where(top, self.c[2] + self.s[2] * lx, np.where(mid, self.c[1] + self.s[1] * lx, self.c[0] + self.s[0] * lx))
            # Y_T (g / b1)^s1 on [b1, b2), Y_T (b2 / b1)^s1 (g / b2)^s2 from b2 on
            more = self.size > 1
            a = np.where(more & (lx >= self.l[1]), self.s[1] * (np.minimum(lx, self.l[2]) - self.l[1]), T(0))
            b = np.where(more & (lx >= self.l[2]), self.s[2] * (lx - self.l[2]), T(0))
            return self.c[0] + a + b

    def Y(self, g):
        with np.errstate(all="ignore"):
            return np.exp2(self.lg2_Y(np.log2(g.astype(self.T))))

    def Y_nu(self, nu):
        with np.errstate(all="ignore"):
            return self.Y(np.sqrt(self.T(K_SYN_GAMMA) * (nu.astype(self.T) / self.B)))

    def stored(self):
        """[n][9]: the three (slope, lg2_lower, lg2_const) as icy_store writes them."""
        cols = []
        for i in range(3):
            live = i < self.size
            cols += [np.where(live, self.s[i], 0), np.where(live, self.l[i], np.inf), np.where(live, self.c[i], 0)]
        return np.stack(cols, axis=1)


def _icy_out(T, rows, side=None, mut=()):
    gm, gc, p, B, YT, kn = (rows[:, j] for j in range(6))
    y = Icy(T, gm, p, B, mut).build(gc, YT, kn != 0, side)
    out = np.concatenate([np.stack([y.gm_hat, y.gc_hat, y.self_, y.regime.astype(T), y.size.astype(T)], axis=1), y.stored(),
                          np.stack([y.Y(rows[:, 6]), y.Y(rows[:, 7]), y.Y_nu(rows[:, 8]), y.Y_nu(rows[:, 9])], axis=1)], axis=1)
    return out, y


def f64_icy(rows, mut=()):
    return _icy_out(np.float64, rows, None, mut)[0]


# ================================================================ one pass of each fixed point (inverse-compton.cpp:192-251)
def _thomson_Y(T, eob, p, gc, gm, lg2_ratio=None, mut=()):
    """compute_Thomson_Y: Y_T = (sqrt(1 + 4 eta_e eps_e / eps_B) - 1) / 2, eta_e = (gamma_c / gamma_m)^(2 - p) above gamma_m, 1 below."""
    with np.errstate(all="ignore"):
        if T is np.float64:
            eta = np.where(gc < gm, 1.0, np.exp2((2 - p) * lg2_ratio))
        else:
            eta = np.where(gc < gm, T(1), (gc / gm) ** (2 - p))
        if T is np.float64:
            return 0.5 * (np.sqrt(4 * eob * eta + 1) - 1)
        x = eob * eta
        return 2 * x / (np.sqrt(4 * x + 1) + 1)  # the same number, without the subtraction that costs long double its digits at small x


def _gamma_c_of(T, t, B, Y, mut=()):
    with np.errstate(all="ignore"):
        gbar = T(er.K_GAMMA_BAR) / (B * B * (1 + Y) * t)
        return (gbar + np.sqrt(gbar * gbar + (0 if "gamma_c_without_plus_4" in mut else 4))) * T(0.5)


def _gamma_M_of(T, B, Y):
    with np.errstate(all="ignore"):
        return np.where(B == 0, np.inf, np.sqrt(T(er.K_GAMMA_M) / np.where(B == 0, 1, B * (1 + Y))))


def _pass(T, t, B, gm, gc, p, eob, kn, mut=()):
    """One pass of gamma_c's fixed point at gc: (Y_T, Y(gc), the next gamma_c, the Y(gamma) it was built on)."""
    t, B, gm, gc, p, eob = (v.astype(T) for v in (t, B, gm, gc, p, eob))
    y = Icy(T, gm, p, B, mut)
    with np.errstate(all="ignore"):
        lg2_gc = np.log2(gc)
        YT = _thomson_Y(T, eob, p, gc, gm, lg2_gc - y.lg2_gm, mut)
        y.build(gc, YT, kn)
        Y = np.where(kn, np.exp2(y.lg2_Y(lg2_gc)), YT)
    return YT, Y, _gamma_c_of(T, t, B, Y, mut), y


def _step_out(T, rows, mut=()):
    t, B, gm, gc, p, eob, kn, gM = (rows[:, j] for j in range(8))
    YT, Y, gc_new, y = _pass(T, t, B, gm, gc, p, eob, kn != 0, mut)
    B = B.astype(T)
    return np.stack([YT, Y, gc_new, _gamma_M_of(T, B, Y), _gamma_M_of(T, B, y.Y(gM))], axis=1)


def f64_step(rows, mut=()):
    return _step_out(np.float64, rows, mut)


def yt_class(YT):
    """sqrt(1 + 4x) - 1 cancels as 1 / x, so the figure of Y_T follows 1 / Y_T: from 1e-3, and below it by decade (down to 1e-14)."""
    YT = np.asarray(YT, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.clip(np.floor(np.log10(np.where(YT > 0, YT, 1e-15))), -15, -4).astype(int)
    return np.where(YT >= 1e-3, "Y_T>=1e-3", np.char.add("Y_T<1e", (d + 1).astype(str)))


# ================================================================ the loops (update_gamma_c_KN, update_gamma_c_Thomson, update_gamma_M)
def stop_margin():
    """delta of the admissible-iterate rule.  A stopping decision compares |x' - x| / x with 1e-3; an error eps in x' (one pass's ceiling)
    and as much carried in x move that quotient by up to 2 eps, i.e. by 2 eps / 1e-3 of the threshold."""
    return 2 * ceiling("step.gc_new") / STOP


def gamma_c_iterates(T, rows, delta, mut=()):
    """Every stopping iterate of ic_gamma_c_cell the rule admits, in arithmetic T: a list of (admitted [n] bool, gc, gc_used, Y_T, passes),
    one entry per pass count, and `guard` [n]: rows that reach the loop's guard without a step below 1e-3 (1 - delta).  delta = 0 with
    float64 is the loop as the device runs it."""
    t, B, gm, stored, last, p, eob, kn = (rows[:, j].astype(T) if j != 7 else rows[:, j] != 0 for j in range(8))
    n = rows.shape[0]
    res = []
    alive, guard = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        # Thomson, no pass: the cell's own gamma_c against the previous cell's
        step = np.abs((last - stored) / stored)
        y0 = Icy(T, gm, p, B)
        YT0 = _thomson_Y(T, eob, p, stored, gm, np.log2(stored) - y0.lg2_gm)
        adm = ~kn & (step <= STOP * (1 + delta))
        res.append((adm, last, last, YT0, np.zeros(n)))
        alive = kn | (step > STOP * (1 - delta))
        x = last
        for j in range(100 if kn.all() else 400):
            if not alive.any():
                break
            YT, Y, xn, _ = _pass(T, t, B, gm, x, p, eob, kn, mut)
            step = np.abs((xn - x) / x)
            last_kn = kn & (j == 99)  # the do-while's guard: the hundredth pass stops whatever its step
            adm = alive & ((step <= STOP * (1 + delta)) | last_kn)
            guard |= alive & last_kn & (step > STOP * (1 + delta))
            res.append((adm, xn, np.where(kn, x, xn), YT, np.full(n, j + 1.0)))
            alive = alive & (step > STOP * (1 - delta)) & ~last_kn
            x = np.where(alive, xn, x)
    return res, guard | alive


def gamma_M_iterates(T, rows, gc_used, YT, delta):
    """The same for ic_gamma_M on the Y(gamma) built from (gc_used, Y_T): a list of (admitted, gM, passes)."""
    t, B, gm, stored, last, p, eob, kn = (rows[:, j].astype(T) if j != 7 else rows[:, j] != 0 for j in range(8))
    y = Icy(T, gm, p, B).build(np.asarray(gc_used), np.asarray(YT), kn)
    n = rows.shape[0]
    res, alive = [], np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        x = rows[:, 8].astype(T)
        for j in range(400):
            if not alive.any():
                break
            xn = _gamma_M_of(T, B, y.Y(x))
            step = np.abs((x - xn) / xn)
            res.append((alive & (step <= STOP * (1 + delta)), x, np.full(n, float(j))))
            alive = alive & (step > STOP * (1 - delta))
            x = np.where(alive, xn, x)
    return res, alive


def chain_errors(t_comv, B, gamma_m, gamma_c, p, eob, kn):
    """The chain vag_ic_cooling_kernel walks, from what Model.details shows of it ([rows][nt], code units): for every cell k >= 1 the
    long-double iteration started from the producer's own gamma_c[k - 1]; the relative distance of gamma_c[k] from the nearest admitted
    stopping iterate (inf where there is none).  The cell's own synchrotron-only gamma_c, which the Thomson loop's first comparison
    reads and the details no longer hold, is formed again from t_comv and B."""
    sh = t_comv[:, 1:].shape
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)
    t, Bf = flat(t_comv[:, 1:]), flat(B[:, 1:])
    rows = np.stack([t, Bf, flat(gamma_m[:, 1:]), _gamma_c_of(LDT, ld(t), ld(Bf), LDT(0)).astype(np.float64), flat(gamma_c[:, :-1]),
                     np.full(t.size, p), np.full(t.size, eob), np.full(t.size, float(kn)), np.ones(t.size)], axis=1)
    res, guard = gamma_c_iterates(LDT, rows, stop_margin())
    got = flat(gamma_c[:, 1:])
    err = np.full(t.size, np.inf)
    for adm, gc, used, YT, passes in res:
        err = np.where(adm, np.minimum(err, rel(got, gc)), err)
    return err.reshape(sh), guard.reshape(sh)


def f64_fixed(rows, mut=()):
    """The loops in float64 as the device runs them: {gc, gc_used, Y_T, passes, gM, passes}."""
    out = np.full((rows.shape[0], 6), np.nan)
    res, _ = gamma_c_iterates(np.float64, rows, 0.0, mut)
    for adm, gc, used, YT, passes in res:
        first = adm & np.isnan(out[:, 0])
        out[first, :4] = np.stack([gc, used, YT, passes], axis=1)[first]
    res, _ = gamma_M_iterates(np.float64, rows, out[:, 1], out[:, 2], 0.0)
    for adm, gM, passes in res:
        first = adm & np.isnan(out[:, 4])
        out[first, 4:] = np.stack([gM, passes], axis=1)[first]
    return out


def fixed_errors(rows, out):
    """A producer's {gc, gc_used, Y_T, passes, gM, passes} against the admitted stopping iterates of the long-double iteration from the same
    start: per quantity the relative error against the iterate with the PRODUCER'S pass count (inf where the rule does not admit that
    count), and how many iterates each row admits.  gamma_M's Y(gamma) is built from the producer's own gc_used and Y_T, the doubles the
    kernel stores between its two stages."""
    delta = stop_margin()
    n = rows.shape[0]
    err = {q: np.full(n, np.inf) for q in ("fixed.gc", "fixed.gc_used", "fixed.Y_T", "fixed.gM")}
    res, guard = gamma_c_iterates(LDT, rows, delta)
    count = np.zeros(n, dtype=int)
    for adm, gc, used, YT, passes in res:
        count += adm
        hit = adm & (out[:, 3] == passes)
        for q, j, ref in (("fixed.gc", 0, gc), ("fixed.gc_used", 1, used), ("fixed.Y_T", 2, YT)):
            err[q] = np.where(hit, rel(out[:, j], ref), err[q])
    res, guard_M = gamma_M_iterates(LDT, rows, out[:, 1], out[:, 2], delta)
    count_M = np.zeros(n, dtype=int)
    for adm, gM, passes in res:
        count_M += adm
        err["fixed.gM"] = np.where(adm & (out[:, 5] == passes), rel(out[:, 4], gM), err["fixed.gM"])
    return err, dict(count=count, count_M=count_M, guard=guard, guard_M=guard_M)


# ================================================================ syn_gamma_a_ic (synchrotron.cpp:212-246) and determine_regime
GA_NEAR = 1e-12  # nu_a is 2^(b log2 a) with |log2 a| up to a few hundred: a comparison of it within this of its threshold goes both ways
LEAVES = ("nu_a <= nu_peak", "slow, nu_a <= nu_c", "slow, nu_a > nu_c", "fast, nu_a <= nu_m", "fast, nu_a > nu_m")


def determine_regime(a, c, m):
    r = np.zeros(np.shape(a), dtype=int)
    for k, cond in reversed(((1, (a <= m) & (m <= c)), (2, (m <= a) & (a <= c)), (3, (a <= c) & (c <= m)), (4, (c <= a) & (a <= m)),
                             (5, (m <= c) & (c <= a)), (6, (c <= m) & (m <= a)))):
        r = np.where(cond, k, r)
    return r


def _gamma_a(T, rows, side=None, mut=()):
    """(gamma_a, Y_c, leaf of the ladder) in arithmetic T; `side`: {"peak" / "c" / "m": -1 / +1}, how nu_a > nu_peak, nu_c, nu_m are
    decided where nu_a is within GA_NEAR of them."""
    B, cd, gm, gc, used, p, YT = (rows[:, j].astype(T) for j in range(7))
    kn = rows[:, 7] != 0
    y = Icy(T, gm, p, B).build(used, YT, kn)
    side = side or {}

    def gt(v, thr, name):
        c = v > thr
        if name in side:
            c = np.where(np.abs((v / thr - 1).astype(np.float64)) <= GA_NEAR, side[name] > 0, c)
        return c

    with np.errstate(all="ignore"):
        pw = (lambda a, b: np.exp2(b * np.log2(a))) if T is np.float64 else (lambda a, b: a ** b)
        Yc = y.Y(gc)
        I = B * T(mr.K_SYN_P) * cd / T(4 * mr.C_PI)
        freq = lambda g: T(mr.K_SYN_FREQ) * B * g * g
        g_peak = np.minimum(gm, gc)
        nu_peak, nu_m, nu_c = freq(g_peak), freq(gm), freq(gc)
        kT = (g_peak - 1) * T(mr.C_ME * mr.C_C2) / 3
        x = I * T(mr.C_C2) / (2 * kT)
        ic = lambda nu, e: pw((1 + Yc) / (1 + y.Y_nu(nu)), e)
        a0 = pw(I * T(mr.C_C2) / (np.cbrt(nu_peak) * 2 * kT), T(0.6))
        e4, e5 = 2 / (p + 4), 2 / (p + 5)
        s1 = pw(x * pw(nu_m, p / 2), e4)
        hi = pw(x * np.sqrt(nu_c) * pw(nu_m, p / 2), e5)
        hi = hi if "gamma_a_without_ic_factor" in mut else hi * ic(hi, e5)
        f1 = pw(x * np.sqrt(nu_c), T(0.4))
        f1 = f1 * ic(f1, T(0.4))
        thick = gt(a0, nu_peak, "peak")
        slow = gc > gm
        s_hi, f_hi = gt(s1, nu_c, "c"), gt(f1, nu_m, "m")
        nu_a = np.where(~thick, a0, np.where(slow, np.where(s_hi, hi, s1), np.where(f_hi, hi, f1)))
        leaf = np.where(~thick, 0, np.where(slow, np.where(s_hi, 2, 1), np.where(f_hi, 4, 3)))
        ga = np.sqrt(T(K_SYN_GAMMA) * (nu_a / B)) + (0 if "gamma_a_without_plus_1" in mut else 1)
    return ga, Yc, leaf


def f64_gamma_a(rows, mut=()):
    ga, Yc, _ = _gamma_a(np.float64, rows, None, mut)
    return np.stack([ga, Yc, determine_regime(ga, rows[:, 3], rows[:, 2]).astype(float), determine_regime(rows[:, 8], rows[:, 9], rows[:, 10]).astype(float)], axis=1)


def ref_gamma_a(rows):
    """[(gamma_a, Y_c)] over the ladder's admitted decisions."""
    res = [_gamma_a(LDT, rows)[:2]]
    for a in (-1, 1):
        for b in (-1, 1):
            for c in (-1, 1):
                res.append(_gamma_a(LDT, rows, dict(peak=a, c=b, m=c))[:2])
    return res


# ================================================================ the same closed forms in mpmath (KN_DPS digits), one row at a time,
# in linear space and from the formulas alone: what tests/test_ic_state_host.py holds the long-double restatements above to.  The
# physical constants enter as the doubles the engine folds them to (K_SYN_FREQ, K_HAT, ...): they are data of the formulas, not results.
def _mpf(v):
    if isinstance(v, mpmath.mpf):
        return v
    return mpmath.mpf(float(v)) if np.isfinite(v) else (mpmath.inf if v > 0 else -mpmath.inf)


class IcyMp:
    """InverseComptonY of one cell: gamma_m_hat = max(m_e c^2 / (h nu_m), 1), gamma_self = (gamma_m_hat gamma_m^2)^(1/3), gamma_c_hat =
    max(gamma_self^3 / gamma_c^2, 1); Y(gamma) = Y_T below the first break, then Y_T (gamma / b1)^s1, then Y_T (b2 / b1)^s1 (gamma / b2)^s2,
    with (b1, s1), (b2, s2) = (gamma_c_hat, (p - 3) / 2), (gamma_m_hat, -4/3) where gamma_m < gamma_c and (gamma_m_hat, -1/2),
    (gamma_c_hat, -4/3) otherwise; no breaks without Klein-Nishina."""

    def __init__(self, gm, gc, p, B, YT, kn):
        gm, gc, p, B, YT = (_mpf(v) for v in (gm, gc, p, B, YT))
        self.B, self.YT = B, YT
        nu_m = _mpf(mr.K_SYN_FREQ) * B * gm ** 2
        self.gm_hat = max(_mpf(K_HAT) / nu_m, 1)
        self.self_ = mpmath.cbrt(self.gm_hat * gm ** 2)
        self.gc_hat = max(self.gm_hat * gm ** 2 / gc ** 2, 1)
        third = mpmath.mpf(4) / 3
        if not kn:
            self.regime, self.breaks = 0, []
        elif gm < gc:
            self.regime, self.breaks = 1, [(self.gc_hat, (p - 3) / 2), (self.gm_hat, -third)]
        else:
            self.regime, self.breaks = 2, [(self.gm_hat, -mpmath.mpf(1) / 2), (self.gc_hat, -third)]

    def Y(self, g):
        y = self.YT
        for i, (b, s) in enumerate(self.breaks):
            if g >= b:
                top = min(g, self.breaks[i + 1][0]) if i + 1 < len(self.breaks) else g
                y = y * (top / b) ** s
        return y

    def Y_nu(self, nu):
        return self.Y(mpmath.sqrt(_mpf(K_SYN_GAMMA) * nu / self.B))

    def stored(self):
        """[(slope, log2 lower, log2 constant)] of the segments: log2 Y = constant + slope log2 gamma on each."""
        out = [(mpmath.mpf(0), mpmath.mpf(0), mpmath.log(self.YT, 2))]
        for b, s in self.breaks:
            s0, _, c0 = out[-1]
            lb = mpmath.log(b, 2)
            out.append((s, lb, c0 + s0 * lb - s * lb))
        return out


def icy_mp(row):
    """The 18 outputs of the ic_y probe (slots past the number of segments: 0, inf, 0)."""
    y = IcyMp(*row[:5], row[5] != 0)
    seg = y.stored() + [(mpmath.mpf(0), mpmath.inf, mpmath.mpf(0))] * (3 - len(y.stored()))
    return [y.gm_hat, y.gc_hat, y.self_, y.regime, len(y.stored())] + [v for t in seg for v in t] + \
        [y.Y(_mpf(row[6])), y.Y(_mpf(row[7])), y.Y_nu(_mpf(row[8])), y.Y_nu(_mpf(row[9]))]


def step_mp(row):
    """The 5 outputs of the ic_step probe: compute_Thomson_Y, Y(gamma_c), gamma_c = (gamma_bar + sqrt(gamma_bar^2 + 4)) / 2 with
    gamma_bar = 6 pi m_e c / (sigma_T B^2 (1 + Y) t), gamma_M = sqrt(6 pi e / (sigma_T B (1 + Y)))."""
    t, B, gm, gc, p, eob, kn, gM = row
    tm, Bm, gmm, gcm, pm, em = (_mpf(v) for v in (t, B, gm, gc, p, eob))
    eta = 1 if gc < gm else (gcm / gmm) ** (2 - pm)
    YT = (mpmath.sqrt(1 + 4 * em * eta) - 1) / 2
    if B == 0:
        return [YT, YT, mpmath.inf, mpmath.inf, mpmath.inf]
    y = IcyMp(gm, gc, p, B, YT, kn != 0)
    Y = y.Y(gcm)
    k_bar, k_M = _mpf(er.K_GAMMA_BAR), _mpf(er.K_GAMMA_M)
    gbar = k_bar / (Bm * Bm * (1 + Y) * tm)
    return [YT, Y, (gbar + mpmath.sqrt(gbar * gbar + 4)) / 2, mpmath.sqrt(k_M / (Bm * (1 + Y))), mpmath.sqrt(k_M / (Bm * (1 + y.Y(_mpf(gM)))))]


def gamma_a_mp(row):
    """(gamma_a, Y_c, the least relative distance of a compared nu_a from its threshold) of compute_syn_gamma_a with the IC terms
    (synchrotron.cpp:212-246), every comparison decided exactly."""
    B, cd, gm, gc, used, p, YT, kn = row[:8]
    y = IcyMp(gm, used, p, B, YT, kn != 0)
    Bm, gmm, gcm, pm = _mpf(B), _mpf(gm), _mpf(gc), _mpf(p)
    Yc = y.Y(gcm)
    c2, k_f = _mpf(mr.C_C2), _mpf(mr.K_SYN_FREQ)
    I = Bm * _mpf(mr.K_SYN_P) * _mpf(cd) / _mpf(4 * mr.C_PI)
    freq = lambda g: k_f * Bm * g * g
    peak = min(gmm, gcm)
    nu_peak, nu_m, nu_c = freq(peak), freq(gmm), freq(gcm)
    x = I * c2 / (2 * (peak - 1) * _mpf(mr.C_ME * mr.C_C2) / 3)
    ic = lambda nu, e: ((1 + Yc) / (1 + y.Y_nu(nu))) ** e
    margin = []

    def above(v, thr):
        margin.append(abs(v / thr - 1))
        return v > thr
    # (the exponents 0.6 and 0.4 are the source's double literals: 3/5 exactly would move nu_a = a^0.6 by 0.6 x 3.7e-17 x ln a, 5e-15)
    e06, e04 = _mpf(0.6), _mpf(0.4)
    nu_a = (x / mpmath.cbrt(nu_peak)) ** e06
    if above(nu_a, nu_peak):
        e5 = 2 / (pm + 5)
        both = lambda: (x * mpmath.sqrt(nu_c) * nu_m ** (pm / 2)) ** e5
        if gc > gm:
            nu_a = (x * nu_m ** (pm / 2)) ** (2 / (pm + 4))
            if above(nu_a, nu_c):
                nu_a = both()
                nu_a = nu_a * ic(nu_a, e5)
        else:
            nu_a = (x * mpmath.sqrt(nu_c)) ** e04
            nu_a = nu_a * ic(nu_a, e04)
            if above(nu_a, nu_m):
                nu_a = both()
                nu_a = nu_a * ic(nu_a, e5)
    return mpmath.sqrt(_mpf(K_SYN_GAMMA) * nu_a / Bm) + 1, Yc, min(margin)


def kn_tails_mp(lg2_x):
    """(corr, lg2_corr) of the two closed-form tails at x = 2^lg2_x: 1 - 2x with the two-term logarithm the device states, and
    3/8 (ln 2x + 1/2) / x."""
    x = mpmath.power(2, _mpf(lg2_x))
    if not lg2_x > KN_LG2_XMIN:
        return 1 - 2 * x, -(2 * x + 2 * x * x) / mpmath.log(2)
    a = mpmath.mpf(3) / 8 * (mpmath.log(2 * x) + mpmath.mpf(1) / 2)
    return a / x, mpmath.log(a / x, 2)


# ================================================================ the probe sets: seeded, at most 4096 random + 256 constructed rows each
_SETS = {}


def _set_kn_lut(rng):
    return np.arange(KN_LUT_N, dtype=np.float64)[:, None], np.full(KN_LUT_N, "node")


def _set_kn_corr(rng):
    nan = np.nan
    n = N_RANDOM - 16  # (271 constructed rows: every node and midpoint)
    lx = rng.uniform(KN_LG2_XMIN - 20, KN_LG2_XMAX + 20, n)
    rows = [np.stack([lx - LG2_X_PER_NU, np.full(n, nan)], axis=1)]
    kind = ["random"] * n
    made = []
    node = kn_node_lg2x(np.arange(KN_LUT_N))
    for v in node:  # both ends of every interval: the nodes themselves
        made.append((v - LG2_X_PER_NU, v, "node"))
    for v in 0.5 * (node[:-1] + node[1:]):
        made.append((v - LG2_X_PER_NU, v, "midpoint"))
    for end in (KN_LG2_XMIN, KN_LG2_XMAX):
        for k in (-1, 0, 1):
            made.append((end - LG2_X_PER_NU, float(nudge(end, k)), "end"))
            made.append((float(nudge(end - LG2_X_PER_NU, k)), nan, "end"))  # the first form's own sum, one step of lg2_nu either side
    for v in (KN_LG2_XMIN - 20, KN_LG2_XMAX + 20):
        made.append((v - LG2_X_PER_NU, v, "20 octaves"))
    made.append((-np.inf, -np.inf, "x = 0"))
    made.append((-np.inf, nan, "x = 0"))
    assert len(made) <= 256 + 24
    rows.append(np.array([m[:2] for m in made], dtype=np.float64))
    kind += [m[2] for m in made]
    return np.concatenate(rows), np.array(kind)


def _set_table(rng):
    """Rows {n, first, th_min, th_max, x, 16 words}: log2 I words in [-200, -50] (no value near zero for a relative metric), NaN from word
    n on so that a read past the table shows."""
    rows, kind = [], []

    def row(n, first, x, k, margin=3.0, words=None):
        last = float(tab_last(first, n, False)) if n >= 1 else first
        w = rng.uniform(-200, -50, TAB_WORDS) if words is None else words.copy()
        w[max(n, 0):] = np.nan
        rows.append(np.concatenate([[n, first, min(first, last) - margin, max(first, last) + margin, x], w]))
        kind.append(k)

    for _ in range(N_RANDOM - 512):
        n = int(rng.choice([2, 3, 16]))
        first = rng.uniform(20, 80)
        row(n, first, first + rng.uniform(0, 2 * IC_Q * (n - 1)), "random")
    for _ in range(512):  # all six n, x anywhere from below the theoretical range to above it
        n = int(rng.choice([-1, 0, 1, 2, 3, 16]))
        first = rng.uniform(20, 80)
        row(n, first, first + rng.uniform(-5, 2 * IC_Q * 15 + 5), "anywhere")
    for n in (-1, 0, 1, 2, 3, 16):
        first = rng.uniform(20, 80)
        last = float(tab_last(first, n, False))
        row(n, first, first, "first")
        for q in range(max(n, 0)):
            row(n, first, float(tab_last(first, q + 1, False)), "node")
        for k in (-2, -1, 0, 1, 2, 4):
            row(n, first, float(nudge(last, k)), "last" if k == 0 else f"last{k:+d}")
        row(n, first, first - 1.0, "th_min < x < first")
        row(n, first, max(first, last) + 1.0, "last < x < th_max")
        row(n, first, first - 4.0, "x < th_min")
        row(n, first, max(first, last) + 4.0, "x > th_max")
        row(n, first, first - 3.0, "x = th_min")
        row(n, first, max(first, last) + 3.0, "x = th_max")
    for n in (2, 3, 16):  # x on the last node: frac = 1 in interval n - 2
        for _ in range(32):
            first = rng.uniform(20, 80)
            row(n, first, float(tab_last(first, n, False)), "last")
        for _ in range(8):
            first = rng.uniform(20, 80)
            row(n, first, first - rng.uniform(0.1, 2.9), "th_min < x < first")
    assert len(rows) <= N_RANDOM + 256
    return np.array(rows), np.array(kind)


def _bin_rows(f_lo, nu_lo, lg2r, d):
    """A consistent power-law bin: f_hi = f_lo 2^d, nu_hi = nu_lo 2^lg2r, the logarithms and the reciprocal as doubles; trap as the
    trapezoid a caller would hand in."""
    f_hi, nu_hi = f_lo * np.exp2(d), nu_lo * np.exp2(lg2r)
    l_lo = np.log2(f_lo)
    return np.stack([f_lo, f_hi, nu_lo, nu_hi, l_lo, l_lo + d, lg2r, 1.0 / lg2r, 0.5 * (f_lo + f_hi) * (nu_hi - nu_lo)], axis=1)


def _set_bin(rng):
    n = N_RANDOM
    s1 = _logu(rng, 1e-3, 1e3, n) * rng.choice([-1.0, 1.0], n)
    lg2r = np.minimum(rng.uniform(0.05, 1.0, n), 60.0 / np.abs(s1 - 1))  # f_hi / f_lo within 2^+-60
    rows = [_bin_rows(_logu(rng, 1e-30, 1e10, n), _logu(rng, 1e-10, 1e10, n), lg2r, (s1 - 1) * lg2r)]
    kind = ["random"] * n
    m = 32
    for sgn in (1.0, -1.0):
        # inv_lg2r = 1: s1 = 1 + d exactly, on the grid of 2^-53 around -+1e-3; k steps of d either side of the threshold
        for k in (-2, -1, 0, 1, 2):
            d = nudge(sgn * 1e-3 - 1.0, k)
            rows.append(_bin_rows(np.ones(8), _logu(rng, 1e-5, 1e5, 8), np.ones(8), np.full(8, d)))
            kind += [f"s1 on the grid at {sgn * 1e-3:+g}"] * 8
        # a general lg2r: the product (lg2f_hi - lg2f_lo) inv_lg2r rounds, the decision is within a rounding of the threshold
        lr = rng.uniform(0.05, 1.0, m)
        r = _bin_rows(np.ones(m), np.ones(m), lr, (sgn * 1e-3 - 1.0) * lr)
        rows.append(r)
        kind += [f"s1 within a rounding of {sgn * 1e-3:+g}"] * m
    lr = rng.uniform(0.05, 1.0, 64)  # inside the series branch
    rows.append(_bin_rows(_logu(rng, 1e-30, 1e10, 64), _logu(rng, 1e-10, 1e10, 64), lr,
                          (_logu(rng, 1e-8, 9e-4, 64) * rng.choice([-1.0, 1.0], 64) - 1.0) * lr))
    kind += ["series"] * 64
    z = _bin_rows(_logu(rng, 1e-20, 1, 24), np.ones(24), np.full(24, 0.4), rng.uniform(-2, 2, 24))
    z[:8, 0], z[8:16, 1] = 0.0, 0.0
    z[16:20, 0], z[20:24, 1] = -1.0, np.nan
    z[:, 8] = rng.uniform(1, 2, 24) * 1e-7
    rows.append(z)
    kind += ["f_lo = 0"] * 8 + ["f_hi = 0"] * 8 + ["f not positive"] * 8
    rows = np.concatenate(rows)
    assert rows.shape[0] <= N_RANDOM + 256
    return rows, np.array(kind)


def _set_scan(rng):
    waves = []
    kind = []
    for _ in range(8):
        waves.append(10.0 ** rng.uniform(-15, 15, 256))
        kind.append("random")
    for hot in (0, 1, 3, 4, 127, 128, 251, 252, 255):
        w = np.zeros(256)
        w[hot] = rng.uniform(1, 2)
        waves.append(w)
        kind.append("one-hot")
    waves.append(np.zeros(256))
    kind.append("zero")
    waves.append(np.full(256, 0.1))
    kind.append("equal")
    rows = np.concatenate(waves).reshape(-1, 4)
    return rows, np.repeat(np.array(kind), 64)


def _set_column(rng):
    n = N_RANDOM
    gm = _logu(rng, 1.5, 1e5, n)
    g = gm * _logu(rng, 1, 1e8, n)
    # (gamma_c / gamma and gamma / gamma_M at most 100: e^-100 is still a normal double)
    gc = np.where(rng.random(n) < 0.5, np.minimum(gm * _logu(rng, 1e-2, 1e4, n), 100 * g), g * _logu(rng, 1e-6, 1e2, n))
    gM = np.where(rng.random(n) < 0.1, np.inf, g * _logu(rng, 0.01, 1e4, n))
    p = rng.choice([2.01, 2.3, 2.999, 3.0, 3.5], n)
    regime = rng.integers(0, 7, n).astype(np.float64)
    rows = np.stack([g, gm, gc, gM, p, regime, _logu(rng, 1e-10, 1e30, n), _logu(rng, 1e-8, 1e4, n), _logu(rng, 1e-8, 1e4, n)], axis=1)
    kind = np.full(n, "random", dtype=object)
    made = rows[:252].copy()
    mk = []
    for j in range(252):
        k = (-1, 0, 1)[j % 3]
        made[j, 5] = float(1 + (j // 3) % 6)
        made[j, 2] = made[j, 0]
        made[j, 0] = float(nudge(made[j, 0], k))  # gamma one step below gamma_c, on it, one step above
        mk.append(("gamma < gamma_c", "gamma = gamma_c", "gamma > gamma_c")[j % 3])
    return np.concatenate([rows, made]), np.concatenate([kind, np.array(mk, dtype=object)]).astype(str)


P_SET = (2.01, 2.3, 2.999, 3.0, 3.5)


def _icy_rows(rng, n):
    gm = _logu(rng, 2, 1e5, n)
    B = _logu(rng, 1e-6, 1e4, n)
    gc = np.maximum(gm * _logu(rng, 1e-3, 1e4, n), 1.5)
    rows = np.stack([gm, gc, rng.choice(P_SET, n), B, _logu(rng, 1e-8, 1e4, n), rng.integers(0, 2, n).astype(float),
                     _logu(rng, 1, 1e9, n), np.ones(n), B * _logu(rng, 1, 1e9, n) ** 2 / K_SYN_GAMMA, B * _logu(rng, 1, 1e9, n) ** 2 / K_SYN_GAMMA], axis=1)
    return rows


def _on_breaks(rows, rng):
    """g1 (column 7) on a break of the row's own Y(gamma) and 1, 2 steps either side; rows without a break keep a random g1."""
    y = _icy_out(np.float64, rows)[1]
    which = rng.integers(1, 3, rows.shape[0])
    lower = np.where(which == 1, y.l[1], y.l[2])
    g = np.exp2(lower)
    k = rng.integers(-2, 3, rows.shape[0])
    for step in (-2, -1, 1, 2):
        g = np.where(k == step, nudge(np.exp2(lower), step), g)
    rows[:, 7] = np.where((rows[:, 5] != 0) & np.isfinite(g), g, _logu(rng, 1, 1e9, rows.shape[0]))
    return rows


def _set_icy(rng):
    rows = _icy_rows(rng, N_RANDOM)
    kind = ["random"] * N_RANDOM
    made = _icy_rows(rng, 240)
    mk = []
    made[:, 5] = 1.0
    made[:, 2] = np.tile(P_SET, 48)
    for j in range(240):
        if j < 60:  # gamma_c on gamma_m and one step either side
            k = (-1, 0, 1)[j % 3]
            made[j, 1] = float(nudge(made[j, 0], k))
            mk.append(("gamma_c < gamma_m", "gamma_c = gamma_m", "gamma_c > gamma_m")[j % 3])
        else:  # the two hats clamped at 1 or not: m_e c^2 / (h nu_m) and gamma_self^3 / gamma_c^2 a decade either side of 1
            m_raw, c_raw = ((10.0, 10.0), (10.0, 0.1), (0.1, 10.0), (0.1, 0.1))[j % 4]
            made[j, 3] = K_HAT / (mr.K_SYN_FREQ * made[j, 0] ** 2 * m_raw)
            made[j, 1] = np.sqrt(max(m_raw, 1.0) * made[j, 0] ** 2 / c_raw)
            made[j, 8:] = made[j, 3] * rng.uniform(1, 1e9, 2) ** 2 / K_SYN_GAMMA
            mk.append(f"hats {'free' if m_raw > 1 else 'clamped'} {'free' if c_raw > 1 else 'clamped'}")
    rows = _on_breaks(np.concatenate([rows, made]), rng)
    return rows, np.array(kind + mk)


def _step_rows(rng, n):
    gm = _logu(rng, 2, 1e5, n)
    B = _logu(rng, 1e-6, 1e4, n)
    gc = np.maximum(gm * _logu(rng, 1e-3, 1e4, n), 1.5)
    t = er.K_GAMMA_BAR / (B * B * _logu(rng, 1e-3, 1e7, n))
    return np.stack([t, B, gm, gc, rng.choice(P_SET, n), _logu(rng, 1e-3, 1e5, n), rng.integers(0, 2, n).astype(float),
                     np.sqrt(er.K_GAMMA_M / B) * _logu(rng, 1e-2, 1, n)], axis=1)


def _set_step(rng):
    rows = _step_rows(rng, N_RANDOM)
    made = _step_rows(rng, 128)
    made[:64, 1] = 0.0  # B = 0: the library fall-backs of ic_rcp and ic_sqrt, gamma_M = inf
    made[:64, 7] = _logu(rng, 1e3, 1e9, 64)
    mk = ["B = 0"] * 64
    for j in range(64, 128):
        k = (-1, 0, 1)[j % 3]
        made[j, 6] = 1.0
        made[j, 3] = float(nudge(made[j, 2], k))
        mk.append(("gamma_c < gamma_m", "gamma_c = gamma_m", "gamma_c > gamma_m")[j % 3])
    small = _step_rows(rng, 48)  # Y_T between 1e-9 and 1e-7, where sqrt(1 + 4x) - 1 keeps 7 to 9 digits
    small[:, 4], small[:, 5] = 3.5, _logu(rng, 1e-3, 1e-2, 48)
    small[:, 3] = small[:, 2] * _logu(rng, 1e3, 1e4, 48)
    return np.concatenate([rows, made, small]), np.array(["random"] * N_RANDOM + mk + ["small Y_T"] * 48)


def _fixed_answer(rows):
    """gamma_c's fixed point itself, iterated far past the stopping rule (float64)."""
    t, B, gm, stored, last, p, eob, kn = (rows[:, j] if j != 7 else rows[:, j] != 0 for j in range(8))
    x = stored
    for _ in range(300):
        x = _pass(np.float64, t, B, gm, x, p, eob, kn)[2]
    return x


def _fixed_rows(rng, n):
    gm = _logu(rng, 2, 1e5, n)
    B = _logu(rng, 1e-6, 1e4, n)
    t = er.K_GAMMA_BAR / (B * B * _logu(rng, 2, 1e7, n))
    stored = _gamma_c_of(np.float64, t, B, 0.0)
    rows = np.stack([t, B, gm, stored, stored, rng.choice(P_SET, n), _logu(rng, 1e-3, 1e5, n), rng.integers(0, 2, n).astype(float),
                     np.sqrt(er.K_GAMMA_M / B) * _logu(rng, 1e-3, 1e3, n)], axis=1)
    return rows


def _set_fixed(rng):
    """Starts 1e-3 ... 1e3 times the answer; rows that converge in one pass; rows whose deciding step lands on 1e-3 to long-double
    precision (two admissible iterates).  Draws whose iteration does not settle (the reference would reach a guard) are not kept: that is
    a condition on the set, checked by the host test."""
    pool = _fixed_rows(rng, 3 * N_RANDOM)
    ans = _fixed_answer(pool)
    pool[:, 4] = np.maximum(ans * _logu(rng, 1e-3, 1e3, pool.shape[0]), 1.01)
    res, guard = gamma_c_iterates(LDT, pool, 1e-9)
    settles = ~guard & np.isfinite(ans) & (np.abs(_pass(np.float64, *(pool[:, j] for j in (0, 1, 2)), ans, pool[:, 5], pool[:, 6], pool[:, 7] != 0)[2] / ans - 1) < 1e-9)
    settles &= np.array([r[0] for r in res[:60]]).any(axis=0)
    pool, ans = pool[settles], ans[settles]
    rows, made, a = pool[:N_RANDOM - 128], pool[N_RANDOM - 128:N_RANDOM].copy(), ans[N_RANDOM - 128:N_RANDOM]
    assert made.shape[0] == 128
    made[:64, 4] = a[:64] * (1 + 1e-5)
    # the deciding step on the threshold: bisect u in last = answer (1 + u) for |F(last) - last| / last = 1e-3
    m, am = made[64:], ld(a[64:])
    t, B, gm, p, eob, kn = (m[:, j] for j in (0, 1, 2, 5, 6, 7))
    lo, hi = np.full(64, LDT(1e-7)), np.full(64, LDT(1.0))

    def g(u):
        x = am * (1 + u)
        return np.abs((_pass(LDT, t, B, gm, x, p, eob, kn != 0)[2] - x) / x) - STOP
    ok = (g(lo) < 0) & (g(hi) > 0)
    for _ in range(90):
        mid = (lo + hi) / 2
        up = g(mid) > 0
        lo, hi = np.where(up, lo, mid), np.where(up, mid, hi)
    m[:, 4] = np.where(ok, (am * (1 + lo)).astype(np.float64), m[:, 4])
    kind = ["random"] * rows.shape[0] + ["one pass"] * 64 + ["on the threshold" if o else "random" for o in ok]
    return np.concatenate([rows, made]), np.array(kind)


def _ga_rows(rng, n):
    gm = _logu(rng, 2, 1e5, n)
    B = _logu(rng, 1e-6, 1e4, n)
    gc = np.maximum(gm * _logu(rng, 1e-3, 1e4, n), 1.5)
    return np.stack([B, _logu(rng, 1e10, 1e70, n), gm, gc, gc * rng.uniform(0.999, 1.001, n), rng.choice(P_SET, n), _logu(rng, 1e-8, 1e4, n),
                     rng.integers(0, 2, n).astype(float), _logu(rng, 1, 1e6, n), _logu(rng, 1, 1e6, n), _logu(rng, 1, 1e6, n)], axis=1)


def _set_gamma_a(rng):
    """Random cells over a column density wide enough for every leaf of the ladder, topped up to 64 rows of each leaf; and for
    determine_regime on its own three numbers all six orderings and every tie of two or three."""
    rows = _ga_rows(rng, N_RANDOM)
    pool = _ga_rows(rng, 8 * N_RANDOM)
    leaf = _gamma_a(np.float64, pool)[2]
    top = np.concatenate([pool[leaf == k][:8] for k in range(5)])
    assert top.shape[0] == 40
    v = _logu(rng, 1, 1e6, (208, 3))
    v.sort(axis=1)
    lo, mid, hi = v[:, 0], v[:, 1], v[:, 2]
    orders = [(lo, hi, mid), (mid, hi, lo), (lo, mid, hi), (mid, lo, hi), (hi, mid, lo), (hi, lo, mid),      # regimes 1 ... 6, strictly
              (lo, lo, hi), (lo, hi, lo), (hi, lo, lo), (hi, hi, lo), (hi, lo, hi), (lo, hi, hi), (lo, lo, lo)]  # ties of two, of three
    made = _ga_rows(rng, 208)
    mk = []
    for j in range(208):
        a, c, m = orders[j % 13]
        made[j, 8:] = a[j], c[j], m[j]
        mk.append("ordering" if j % 13 < 6 else "tie")
    return np.concatenate([rows, top, made]), np.array(["random"] * N_RANDOM + ["leaf"] * 40 + mk)


_MAKERS = {"kn_lut": (_set_kn_lut, 11), "kn_corr": (_set_kn_corr, 12), "ic_table": (_set_table, 13), "ic_bin_integral": (_set_bin, 14),
           "ic_suffix_scan": (_set_scan, 15), "ic_column_den": (_set_column, 16), "ic_y": (_set_icy, 17), "ic_step": (_set_step, 18),
           "ic_fixed_point": (_set_fixed, 19), "ic_gamma_a": (_set_gamma_a, 20)}


def probe_set(name):
    """(rows [n][n_in], kind [n]) of a probe routine.  One fixed seed; cached."""
    if name not in _SETS:
        make, k = _MAKERS[name]
        rows, kind = make(np.random.default_rng([SEED, k]))
        _SETS[name] = (np.ascontiguousarray(rows, dtype=np.float64), kind)
    return _SETS[name]


def f64_out(name, mut=()):
    """The float64 restatement's outputs on probe_set(name), in the probe routine's column order."""
    rows = probe_set(name)[0]
    return {"kn_lut": lambda: f64_kn_lut(rows[:, 0].astype(int)), "kn_corr": lambda: f64_kn_corr(rows, mut),
            "ic_table": lambda: f64_table(rows, mut), "ic_bin_integral": lambda: f64_bin(rows, mut),
            "ic_suffix_scan": lambda: f64_scan(rows, mut), "ic_column_den": lambda: f64_column(rows, mut),
            "ic_y": lambda: f64_icy(rows, mut), "ic_step": lambda: f64_step(rows, mut), "ic_fixed_point": lambda: f64_fixed(rows, mut),
            "ic_gamma_a": lambda: f64_gamma_a(rows, mut)}[name]()


# ================================================================ a producer's outputs against the reference
_REFS = {}


def _refs(name):
    if name not in _REFS:
        rows = probe_set(name)[0]
        _REFS[name] = {"kn_lut": ref_kn_lut_all, "kn_corr": lambda: ref_kn_corr(rows), "ic_table": lambda: ref_table(rows),
                       "ic_bin_integral": lambda: ref_bin(rows), "ic_suffix_scan": lambda: ref_scan(rows),
                       "ic_column_den": lambda: ref_column(rows),
                       "ic_y": lambda: [_icy_out(LDT, rows, sd) for sd in (None, -1, 1)], "ic_step": lambda: _step_out(LDT, rows),
                       "ic_fixed_point": lambda: None, "ic_gamma_a": lambda: ref_gamma_a(rows)}[name]()
    return _REFS[name]


def point_errors(name, out):
    """A producer's outputs `out` [n][n_out] (the float64 restatement's or the device's) on probe_set(name), each value against the nearest
    reference the thresholds admit: {quantity: (relative error [m], class key [m] -- the tuple a ceiling is looked up with, joined with
    ";" -- and the rows [m] compared)}.  `counts` holds what must be zero: outputs that must be exact (breach bits, a trap handed back,
    the zeros and infinities) and are not."""
    rows, kind = probe_set(name)
    out = np.asarray(out, dtype=np.float64)
    every = np.arange(rows.shape[0])
    res, counts = {}, {}

    def put(q, err, classes=(), idx=every):
        key = np.array([";".join((q,) + t) for t in zip(*classes)]) if classes else np.full(np.shape(err), q)
        res[q] = (np.asarray(err, dtype=np.float64), key, idx)

    refs = _refs(name)
    if name == "kn_lut":
        put("lut.ratio", nearest(out[:, 0], [r[0] for r in refs]))
        put("lut.lg2_ratio", nearest(out[:, 1], [r[1] for r in refs]))
    elif name == "kn_corr":
        c1 = kn_class(rows[:, 0] + LG2_X_PER_NU)
        c2 = kn_class(_kn_lg2x(rows))
        for j, (q, c) in enumerate((("lg2.corr", c1), ("lg2.lg2_corr", c1), ("node.corr", c2), ("node.lg2_corr", c2))):
            fin = np.isfinite(refs[0][:, j].astype(np.float64)) & (refs[0][:, j] != 0)
            put(q, nearest(out[fin, j], [r[fin, j] for r in refs]), (c[fin],), every[fin])
            counts[f"{q}: not the reference's 0 / -inf at x = 0"] = int(np.sum(out[~fin, j] != refs[0][~fin, j].astype(np.float64)))
    elif name == "ic_table":
        # the producer formed one `last`: its value and its breach bits must come from the same one
        err = np.full(rows.shape[0], np.inf)
        for v, b in refs:
            inf = ~np.isfinite(v.astype(np.float64))
            e = np.where(inf, np.where(out[:, 0] == v.astype(np.float64), 0.0, np.inf), rel(out[:, 0], np.where(inf, 1, v)))
            err = np.minimum(err, np.where(out[:, 1] == b, e, np.inf))
        fin = np.isfinite(refs[0][0].astype(np.float64)) & np.isfinite(refs[1][0].astype(np.float64))
        put("table.value", err[fin], (), every[fin])
        counts["table: a value or breach bits that no admitted `last` gives"] = int(np.sum(~np.isfinite(err)))
    elif name == "ic_bin_integral":
        cls = bin_class(rows)
        trap = cls == "trap"
        counts["trap not handed back bit for bit"] = int(np.sum(out[trap, 0].view(np.int64) != rows[trap, 8].view(np.int64)))
        put("bin", nearest(out[~trap, 0], [r[~trap] for r in refs]), (cls[~trap],), every[~trap])
    elif name == "ic_suffix_scan":
        zero = refs == 0
        counts["a suffix of zeros that is not zero"] = int(np.sum(out[zero] != 0))
        e = rel(np.where(zero, 1, out), np.where(zero, 1, refs)).max(axis=1)
        put("scan", e)
    elif name == "ic_column_den":
        zero = rows[:, 5] == 0
        counts["regime 0 does not give 0"] = int(np.sum(out[zero, 0] != 0))
        put("column_den", rel(out[~zero, 0], refs[~zero]), (np.where(np.isin(rows[~zero, 5], (1, 2, 5)), "slow", "fast"),), every[~zero])
    elif name == "ic_y":
        def relx(got, ref):  # an infinite reference: the same infinity, exactly
            fin = np.isfinite(ref.astype(np.float64))
            return np.where(fin, rel(got, np.where(fin, ref, 1)), np.where(got == ref.astype(np.float64), 0.0, np.inf))
        o = [r[0] for r in refs]
        for j, q in enumerate(("gamma_m_hat", "gamma_c_hat", "gamma_self")):
            put("icy." + q, np.minimum.reduce([relx(out[:, j], r[:, j]) for r in o]))
        counts["regime or number of segments"] = int(np.sum((out[:, 3] != o[0][:, 3].astype(np.float64)) | (out[:, 4] != o[0][:, 4].astype(np.float64))))
        put("icy.slope", np.maximum.reduce([relx(out[:, 5 + 3 * i], o[0][:, 5 + 3 * i]) for i in range(3)]))
        def lowx(got, ref):  # a break within a factor 2 of gamma = 1 (a hat at its clamp) is held absolutely: |d log2| / max(|log2|, 1)
            fin = np.isfinite(ref.astype(np.float64))
            d = (np.abs(ld(got) - np.where(fin, ref, 0)) / np.maximum(np.abs(np.where(fin, ref, 0)), 1)).astype(np.float64)
            return np.where(fin, np.where(np.isnan(d), np.inf, d), np.where(got == ref.astype(np.float64), 0.0, np.inf))
        put("icy.lg2_lower", np.maximum.reduce([np.minimum.reduce([lowx(out[:, 6 + 3 * i], r[:, 6 + 3 * i]) for r in o]) for i in range(3)]))
        e = []
        for i in range(3):  # the constants against what their subtractions cancel from
            d = [np.abs(ld(out[:, 7 + 3 * i]) - r[:, 7 + 3 * i]) / np.where(y.c_scale[i] == 0, 1, y.c_scale[i]) for r, y in refs]
            live = i < out[:, 4]
            e.append(np.where(live, np.minimum.reduce(d).astype(np.float64), np.where(out[:, 7 + 3 * i] == 0, 0.0, np.inf)))
        put("icy.lg2_const", np.where(np.isnan(np.maximum.reduce(e)), np.inf, np.maximum.reduce(e)))
        put("icy.Y", np.maximum(*[np.minimum.reduce([relx(out[:, j], r[:, j]) for r in o]) for j in (14, 15)]))
        put("icy.Y_nu", np.maximum(*[np.minimum.reduce([relx(out[:, j], r[:, j]) for r in o]) for j in (16, 17)]))
    elif name == "ic_step":
        def relx(got, ref):
            fin = np.isfinite(ref.astype(np.float64))
            return np.where(fin, rel(got, np.where(fin, ref, 1)), np.where(got == ref.astype(np.float64), 0.0, np.inf))
        cls = yt_class(refs[:, 0])
        put("step.Y_T", relx(out[:, 0], refs[:, 0]), (cls,))
        put("step.Y", relx(out[:, 1], refs[:, 1]), (cls,))
        for j, q in ((2, "gc_new"), (3, "gM"), (4, "gM_pass")):
            put("step." + q, relx(out[:, j], refs[:, j]))
    elif name == "ic_fixed_point":
        err, info = fixed_errors(rows, out)
        for q, e in err.items():
            put(q, e, (yt_class(out[:, 2]),) if q == "fixed.Y_T" else ())
        counts["a pass count that the rule does not admit"] = int(np.sum(~np.isfinite(err["fixed.gc"])) + np.sum(~np.isfinite(err["fixed.gM"])))
    elif name == "ic_gamma_a":
        put("ga.gamma_a", nearest(out[:, 0], [r[0] for r in refs]))
        put("ga.Y_c", nearest(out[:, 1], [r[1] for r in refs]))
        # the regime of gamma_a among gamma_c and gamma_m: of some admitted gamma_a, or of one GA_NEAR either side of it
        ok = np.zeros(rows.shape[0], dtype=bool)
        for ga, _ in refs:
            for f in (1.0, 1 - GA_NEAR, 1 + GA_NEAR):
                ok |= determine_regime((ga * LDT(f)).astype(np.float64), rows[:, 3], rows[:, 2]) == out[:, 2]
        counts["a regime that no admitted gamma_a gives"] = int(np.sum(~ok))
        counts["determine_regime on its own three numbers"] = int(np.sum(determine_regime(rows[:, 8], rows[:, 9], rows[:, 10]) != out[:, 3]))
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


# ================================================================ ceilings: 25 x the float64 figure beside each (CPU_FIGURES, measured by
# tests/test_ic_state_host.py on the restatements above with numpy on glibc; that test asserts them again)
CEILING_FACTOR = 25
# The maxima of the float64 restatements over the probe sets, rounded up to two digits.
CPU_FIGURES = {
    # the table's nodes: the float64 Klein-Nishina formula cancels at small x (worst at node 4, x = 0.0134), and log2 of a ratio near 1
    # multiplies that by 1 / |ln ratio|.  The look-ups inherit both inside the table.
    ("lut.ratio",): 2.5e-12, ("lut.lg2_ratio",): 9.3e-11,
    **{(f + q, c): v for f in ("lg2.", "node.") for q, row in (("corr", (7.9e-17, 2.5e-12, 1.5e-15)), ("lg2_corr", (1.5e-15, 9.3e-11, 3.7e-16)))
       for c, v in zip(("below", "table", "above"), row)},
    ("table.value",): 1.4e-15,
    ("bin", "series"): 2.2e-16, ("bin", "s1~1e-3"): 8.2e-13, ("bin", "s1<1e-2"): 2.4e-12, ("bin", "s1<1e-1"): 2.1e-13, ("bin", "s1>=1e-1"): 2.4e-14,
    ("scan",): 4.3e-16,
    ("column_den", "slow"): 2.0e-14, ("column_den", "fast"): 2.0e-14,
    # IcY: everything is carried in log2, so a value 2^e carries |e| roundings (gamma_self, gamma_c_hat, Y); lg2_lower as
    # |d| / max(|lg2_lower|, 1), lg2_const against what its subtractions cancel from
    ("icy.gamma_m_hat",): 3.0e-16, ("icy.gamma_c_hat",): 6.6e-15, ("icy.gamma_self",): 2.2e-15, ("icy.slope",): 5.6e-17,
    ("icy.lg2_lower",): 1.1e-14, ("icy.lg2_const",): 1.8e-15, ("icy.Y",): 8.5e-15, ("icy.Y_nu",): 9.1e-15,
    # one pass: Y_T = (sqrt(1 + 4x) - 1) / 2 cancels as 1 / x, the formula's own figure at small Y_T (by decade: the figure follows
    # 1 / Y_T, down to 4 digits left at 1e-12), and Y(gamma_c) inherits it
    **{("step.Y_T", c): v for c, v in (
        ("Y_T<1e-3", 4.5e-13), ("Y_T<1e-4", 6.1e-12), ("Y_T<1e-5", 5.0e-11), ("Y_T<1e-6", 5.2e-10), ("Y_T<1e-7", 3.2e-09),
        ("Y_T<1e-8", 4.2e-08), ("Y_T>=1e-3", 7.4e-14))},
    **{("step.Y", c): v for c, v in (
        ("Y_T<1e-3", 4.5e-13), ("Y_T<1e-4", 6.1e-12), ("Y_T<1e-5", 5.0e-11), ("Y_T<1e-6", 5.2e-10), ("Y_T<1e-7", 3.2e-09),
        ("Y_T<1e-8", 4.2e-08), ("Y_T>=1e-3", 7.4e-14))},
    ("step.gc_new",): 2.4e-15, ("step.gM",): 2.4e-15, ("step.gM_pass",): 3.7e-15,
    ("fixed.gc",): 3.5e-15, ("fixed.gc_used",): 7.7e-15, ("fixed.gM",): 4.0e-15,
    ("ga.gamma_a",): 8.0e-15, ("ga.Y_c",): 6.4e-15,
    **{("fixed.Y_T", c): v for c, v in (
        ("Y_T<1e-3", 6.2e-13), ("Y_T<1e-4", 7.5e-12), ("Y_T<1e-5", 5.5e-11), ("Y_T<1e-6", 5.2e-10), ("Y_T<1e-7", 4.0e-09),
        ("Y_T<1e-8", 5.2e-08), ("Y_T<1e-9", 3.2e-07), ("Y_T<1e-10", 8.8e-07), ("Y_T<1e-11", 1.4e-05), ("Y_T<1e-12", 1.7e-04),
        ("Y_T>=1e-3", 7.0e-14))},
}
PREFIX = {"kn_lut": ("lut",), "kn_corr": ("lg2", "node"), "ic_table": ("table",), "ic_bin_integral": ("bin",), "ic_suffix_scan": ("scan",),
          "ic_column_den": ("column_den",), "ic_y": ("icy",), "ic_step": ("step",), "ic_fixed_point": ("fixed",), "ic_gamma_a": ("ga",)}


def ceiling(quantity, *cls):
    return CEILING_FACTOR * CPU_FIGURES[(quantity,) + tuple(cls)]


def key_ceilings(keys):
    """The ceiling of every per-point class key of point_errors."""
    return np.array([ceiling(*k.split(";")) for k in keys])
