"""High-precision references of the engine's device math (tests/test_device_math.py) -- the formula each routine claims to implement.

Vectorised in numpy.longdouble (64-bit mantissa on x86-64); mpmath at 40 digits is the cross-check, and the fall-back where longdouble
is no wider than a double.  Inputs are float64 arrays; results are arrays of the backend's type (`to_ld` brings them to longdouble).

* exp2, log2, rcp, sqrt: the exact functions.
* softplus: log2_softplus of the reference (oracle/vag_oracle.c:82): z for z > 20, 0 for z < -20, log2(1 + 2^z) otherwise.
* the synchrotron spectrum: photons_build + compute_log2_I_nu with Y = 0 (vag_oracle.c:2300-2376; device: vag_device.h
  syn_photons_build, log2_I_nu), with the reference's own shortcuts (the +-20 softplus cut, log2_x_far, lg2_nu - l_M < -20) and the
  engine's unit constants as the doubles vag_device.h defines.
Every branch of the spectrum takes a `side`: None decides each threshold comparison exactly; -1 / +1 decide the comparisons within
`THRESH_TOL` of their threshold as if the value sat just below / above it.  A device value computed in double may fall on either side
of such a point, and matches one of the two.
"""
import numpy as np

try:
    import mpmath
except ImportError:  # pragma: no cover - the machine's python decides
    mpmath = None

LD_OK = np.finfo(np.longdouble).nmant >= 63
if not LD_OK and mpmath is None:
    raise ImportError("no high-precision arithmetic: numpy.longdouble is no wider than a double and mpmath is missing")

# ---- the engine's unit constants (vag_device.h:17-40), same expression order => the same doubles ----
U_LEN = 1.5e13
U_CM = 1 / U_LEN
U_SEC = 3e10 / U_LEN
U_G = 1 / 2e33
C_C = 1.0
C_C2 = C_C * C_C
C_MP = 1.67e-24 * U_G
C_ME = C_MP / 1836
C_E = 4.8e-10 / 4.472136e16 / 5.809475e19 / U_SEC
C_E2 = C_E * C_E
C_E3 = C_E2 * C_E
C_PI = 3.14159265358979323846
LN2 = 0.693147180559945309417232121458176568
LOG2E = 1.442695040888963407359924681001892137
SQRT3 = 1.732050807568877293527446341505872367
K_SYN_FREQ = 3 * C_E / (4 * C_PI * C_ME * C_C)  # syn_freq's constant, folded by the compiler in this order
K_SYN_P = (C_PI / 4) * 0.92 * SQRT3 * C_E3 / (C_ME * C_C2)  # syn_I_peak's

THRESH_TOL = 1e-12  # relative to max(1, |value|): comparisons this close to their threshold are decided both ways


class _LongDouble:
    name = "longdouble"

    @staticmethod
    def arr(x):
        return np.asarray(x, dtype=np.float64).astype(np.longdouble)

    @staticmethod
    def const(c):
        return np.longdouble(c)

    exp2 = staticmethod(np.exp2)
    log2 = staticmethod(np.log2)
    log1p = staticmethod(np.log1p)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def log2e():
        return 1 / np.log(np.longdouble(2))


class _Mp:
    name = "mpmath"

    @staticmethod
    def arr(x):
        return np.array([mpmath.mpf(float(v)) for v in np.ravel(np.asarray(x, dtype=np.float64))], dtype=object).reshape(np.shape(x))

    @staticmethod
    def const(c):
        return mpmath.mpf(float(c))

    if mpmath is not None:
        exp2 = staticmethod(np.frompyfunc(lambda v: mpmath.power(2, v), 1, 1))
        log2 = staticmethod(np.frompyfunc(lambda v: mpmath.log(v, 2) if v > 0 else (mpmath.mpf("-inf") if v == 0 else mpmath.mpf("nan")), 1, 1))
        log1p = staticmethod(np.frompyfunc(mpmath.log1p, 1, 1))
        sqrt = staticmethod(np.frompyfunc(mpmath.sqrt, 1, 1))

    @staticmethod
    def log2e():  # at the working precision of the call
        return 1 / mpmath.log(2)


LD = _LongDouble
MP = _Mp
DEFAULT = LD if LD_OK else MP


def to_ld(x):
    """Backend values as longdouble (mpmath values are rounded once, to 64 bits)."""
    x = np.asarray(x)
    if x.dtype == object:
        return np.array([np.longdouble(mpmath.nstr(v, 30)) for v in x.ravel()], dtype=np.longdouble).reshape(x.shape)
    return x.astype(np.longdouble)


def _in(B, x):
    return B.arr(x) if not (isinstance(x, np.ndarray) and x.dtype in (np.longdouble, object)) else x


def _where(c, a, b):
    return np.where(np.asarray(c, dtype=bool), a, b)


def _gt(v, t, side):
    """v > t, with values within THRESH_TOL of t decided as if on `side` of it (None: exactly)."""
    c = np.asarray(v > t, dtype=bool)
    if side is None:
        return c
    near = np.abs(to_float(v - t)) <= THRESH_TOL * np.maximum(1.0, np.abs(to_float(np.asarray(t))))
    return np.where(near, side > 0, c)


def to_float(x):
    x = np.asarray(x)
    return np.array([float(v) for v in x.ravel()]).reshape(x.shape) if x.dtype == object else x.astype(np.float64)


# ---- elementary functions ----
def exp2(x, B=DEFAULT):
    return B.exp2(_in(B, x))


def log2(x, B=DEFAULT):
    return B.log2(_in(B, x))


def rcp(x, B=DEFAULT):
    return 1 / _in(B, x)


def sqrt(x, B=DEFAULT):
    return B.sqrt(_in(B, x))


def log2_1p_exp2(z, B=DEFAULT):
    """log2(1 + 2^z), exact (no shortcut): max(z, 0) + log2(e) log1p(2^-|z|)."""
    z = _in(B, z)
    a = np.abs(z)
    return _where(z > 0, z, np.zeros_like(z)) + B.log2e() * B.log1p(B.exp2(-a))


def softplus(z, B=DEFAULT, side=None):
    """log2_softplus of the reference: z for z > 20, 0 for z < -20, log2(1 + 2^z) otherwise."""
    z = _in(B, z)
    return _where(_gt(z, 20.0, side), z, _where(_gt(-z, 20.0, side), np.zeros_like(z), log2_1p_exp2(z, B)))


# ---- the synchrotron spectrum ----
def _sigmoid2(x, B):
    return 1 / (1 + B.exp2(-x))


def _blend(w, a, b):
    return w * a + (1 - w) * b


def photons_build(nu_m, nu_c, nu_a, nu_M, I_max, p, B=DEFAULT, side=None):
    """SmoothPowerLawSyn::build (vag_oracle.c photons_build) from the break frequencies and peak intensity (internal units)."""
    nu_m, nu_c, nu_a, nu_M, I_max, p = (_in(B, v) for v in (nu_m, nu_c, nu_a, nu_M, I_max, p))
    c = B.const
    ph = dict(p=p, l_I=B.log2(I_max), l_m=B.log2(nu_m), l_c=B.log2(nu_c), l_a=B.log2(nu_a), l_M=B.log2(nu_M), nu_M=nu_M)
    lm, lc, la = ph["l_m"], ph["l_c"], ph["l_a"]
    ph["smooth_thick"] = (c(3.44) * p - c(1.41)) / c(LN2)
    ph["log2_x_far"] = c(1.5) * B.log2(c(20.0) / ph["smooth_thick"])
    w_slow = _sigmoid2(4 * (lc - lm), B)
    soft_offset = softplus(-4 * np.abs(lc - lm), B, side) / 4
    ph["l_lo"] = np.minimum(lm, lc) - soft_offset
    ph["l_hi"] = np.maximum(lm, lc) + soft_offset
    fl = c(0.1)
    s_m_slow = np.maximum(c(1.84) - c(0.40) * p, fl)
    s_c_slow = np.maximum(c(1.15) - c(0.06) * p, fl)
    s_m_fast = np.maximum(c(3.34) - c(0.82) * p, fl)
    ph["smooth_lo"] = _blend(w_slow, s_m_slow, c(0.597))
    ph["smooth_hi"] = _blend(w_slow, s_c_slow, s_m_fast)
    alpha_mid = _blend(w_slow, -(p - 1) / 2, c(-0.5) + 0 * p)
    ph["diff_lo"] = ph["smooth_lo"] * (c(1) / 3 - alpha_mid)
    ph["diff_hi"] = ph["smooth_hi"] * (alpha_mid + p / 2)
    u = _sigmoid2(4 * (la - lm), B)
    v = _sigmoid2(4 * (la - lc), B)
    w_below, w_above = (1 - u) * (1 - v), u * v
    s_a_mid = np.maximum(c(1.47) - c(0.21) * p, fl)
    s_a_above = np.maximum(c(0.94) - c(0.14) * p, fl)
    ph["s_a_blend"] = w_below * c(1.64) + w_above * s_a_above + (1 - w_below - w_above) * s_a_mid
    # the sharp thin / thick forms at nu_a (continuous at every tie, so no side)
    slow = np.asarray(lm < lc, dtype=bool)
    thin_slow = _where(la < lm, (la - lm) / 3, _where(la < lc, (1 - p) / 2 * (la - lm), (1 - p) / 2 * (lc - lm) - p / 2 * (la - lc)))
    thin_fast = _where(la < lc, (la - lc) / 3, _where(la < lm, -(la - lc) / 2, -(lm - lc) / 2 - p / 2 * (la - lm)))
    thin_a = _where(slow, thin_slow, thin_fast)
    thick_a = _where(la < lm, 2 * (la - lm), c(2.5) * (la - lm))
    ph["thick_norm"] = thin_a - thick_a
    return ph


def log2_I_nu(ph, lg2_nu, B=DEFAULT, side=None):
    """compute_log2_I_nu with Y == 0 (vag_oracle.c) on a photons_build result; lg2_nu broadcasts against the cells."""
    x = _in(B, lg2_nu)
    sp = lambda z: softplus(z, B, side)  # noqa: E731
    thin = (x - ph["l_lo"]) / 3 - sp(ph["diff_lo"] * (x - ph["l_lo"])) / ph["smooth_lo"] - \
        sp(ph["diff_hi"] * (x - ph["l_hi"])) / ph["smooth_hi"]
    return _finish(ph, x, thin, B, side)


def _finish(ph, x, thin, B, side):
    sp = lambda z: softplus(z, B, side)  # noqa: E731
    lx = x - ph["l_m"]
    far = _gt(lx, ph["log2_x_far"], side)
    lx_near = _where(far, 0 * lx, lx)  # (the far branch drops the term; keep its argument finite)
    s = -ph["smooth_thick"] * B.exp2(B.const(2) / 3 * lx_near)
    thick = B.const(2.5) * lx + _where(far, 0 * lx, sp(-lx_near / 2 + s))
    lb = thick + ph["thick_norm"]
    smooth_one = thin - sp(ph["s_a_blend"] * (thin - lb)) / ph["s_a_blend"]
    spec = ph["l_I"] + (1 / ph["smooth_lo"] + smooth_one)
    below = _gt(-(x - ph["l_M"]), 20.0, side)  # lg2_nu - l_M < -20
    xe = _where(below, 0 * x, x)
    return _where(below, spec, spec - B.log2e() * B.exp2(xe) / ph["nu_M"])


def breaks_from_physical(gamma_m, gamma_c, gamma_a, gamma_M, column_den, Bf, B=DEFAULT):
    """(nu_m, nu_c, nu_a, nu_M, I_max) of syn_photons_build (syn_freq, syn_I_peak) with the engine's constants."""
    g = [_in(B, v) for v in (gamma_m, gamma_c, gamma_a, gamma_M)]
    Bv, cd = _in(B, Bf), _in(B, column_den)
    k = B.const(K_SYN_FREQ)
    nus = [k * Bv * gi * gi for gi in g]
    I_max = Bv * B.const(K_SYN_P) * cd / B.const(4 * C_PI)
    return nus[0], nus[1], nus[2], nus[3], I_max


def photons_from_physical(gamma_m, gamma_c, gamma_a, gamma_M, column_den, Bf, p, B=DEFAULT, side=None):
    nu_m, nu_c, nu_a, nu_M, I_max = breaks_from_physical(gamma_m, gamma_c, gamma_a, gamma_M, column_den, Bf, B)
    return photons_build(nu_m, nu_c, nu_a, nu_M, I_max, p, B, side)


# ---- the spectrum on a folded cell block (vag_common.h VP_*), with an optional IC thin-branch correction ----
VP = dict(LG2_LO=0, BHI=1, DLO=2, INV_SLO=3, DHI=4, INV_SHI=5, LG2_NUM=6, TB=7, SAB=8, INV_SAB=9, LG2_I_SLO=10, LG2_NUMAX=11,
          INV_NUMAX=12)
NPAR = 18
NQ = 14


def log2_I_nu_block(blk, p, lg2_nu, B=DEFAULT, side=None, thin_add=None):
    """The evaluator's formula on the VAG_NPAR block as the device holds it (blk [n][NPAR] float64): exact softplus with the +-20 cut,
    plus `thin_add` (backend values) on the thin branch."""
    c = {k: _in(B, blk[:, i]) for k, i in VP.items()}
    pv = _in(B, p)
    x = _in(B, lg2_nu)
    sp = lambda z: softplus(z, B, side)  # noqa: E731
    thin = (x - c["LG2_LO"]) / 3 - sp(c["DLO"] * (x - c["LG2_LO"])) * c["INV_SLO"] - sp(c["DHI"] * x + c["BHI"]) * c["INV_SHI"]
    if thin_add is not None:
        thin = thin + thin_add
    smooth_thick = (B.const(3.44) * pv - B.const(1.41)) / B.const(LN2)
    ph = dict(l_m=c["LG2_NUM"], log2_x_far=B.const(1.5) * B.log2(B.const(20.0) / smooth_thick), smooth_thick=smooth_thick,
              thick_norm=c["TB"] + B.const(2.5) * c["LG2_NUM"], s_a_blend=c["SAB"], smooth_lo=1 / c["INV_SLO"],
              l_I=c["LG2_I_SLO"] - c["INV_SLO"], l_M=c["LG2_NUMAX"], nu_M=B.log2e() / c["INV_NUMAX"])
    return _finish(ph, x, thin, B, side)
