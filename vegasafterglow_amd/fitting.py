"""Batched log-likelihood: host-side mirror of the reference's Fitter evaluation path.

Mirrors ``VegasAfterglow/fitting/fitter.py:407-451`` (_consolidate_data), ``:497-533`` (_chi2_sum,
_evaluate), ``fitting/utils.py:110-135`` (transformer), ``fitting/samplers.py:61-91`` (eval_one,
log_prob_batch) for point flux-density data, with the per-walker ``Model`` evaluations replaced by ONE
batched call into the HIP engine (``vag_loglike_batch``).  Sampler drivers (emcee/bilby) stay
third-party: hand ``Fitter.log_prob_batch`` to ``emcee.EnsembleSampler(..., vectorize=True)``.
"""
import ctypes as C
import logging
import math
import re
from dataclasses import dataclass
from enum import Enum
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .model import get_context

logger = logging.getLogger(__name__)
logger.addHandler(logging.NullHandler())

# the registry of VegasAfterglow/fitting/config.py:99-121 ("uniform" = TophatJet with theta_c fixed to pi/2)
JET_TYPES = {"tophat": _lib.JET_TOPHAT, "gaussian": _lib.JET_GAUSSIAN, "powerlaw": _lib.JET_POWERLAW,
             "two_component": _lib.JET_TWO_COMPONENT, "step_powerlaw": _lib.JET_STEP_POWERLAW,
             "powerlaw_wing": _lib.JET_POWERLAW_WING, "uniform": _lib.JET_TOPHAT}
MEDIUM_TYPES = {"ism": _lib.MEDIUM_ISM, "wind": _lib.MEDIUM_WIND}


def logscale_screen(data, data_density):
    """Indices that thin a sorted positive array to about `data_density` points per decade, end points always kept
    (pybind.h:40-107): the targets are log-uniform between data[0] and data[-1], each replaced by the interior sample
    nearest to it in LINEAR distance (first one on ties), duplicates dropped.  Host-side data preparation for a fit."""
    x = np.asarray(data, dtype=np.float64).ravel()
    n, density = x.size, int(data_density)
    if n <= 1:
        return list(range(n))
    if density == 0:
        return list(range(n))
    lo, hi = np.log10(x[0]), np.log10(x[-1])
    n_targets = int(np.ceil((hi - lo) * density)) + 1
    keep = {0, n - 1}
    if n_targets > 2 and n > 2:
        step = (hi - lo) / (n_targets - 1)
        interior = x[1:n - 1]
        for i in range(1, n_targets - 1):
            keep.add(1 + int(np.argmin(np.abs(interior - 10.0 ** (lo + i * step)))))
    elif n_targets > 2:
        keep.add(1)
    return sorted(keep)


class Scale(Enum):
    linear = "linear"
    log = "log"
    fixed = "fixed"


@dataclass
class ParamDef:
    """ParamDef(name, lower, upper, scale, initial) -- VegasAfterglow/types.py."""
    name: str
    lower: float
    upper: float
    scale: Scale = Scale.linear
    initial: Optional[float] = None


# ModelParams defaults, VegasAfterglow/types.py:37-77
MODEL_PARAM_DEFAULTS = dict(theta_v=0.0, n_ism=0.0, n0=math.inf, A_star=0.0, k_m=2.0, E_iso=1e52, Gamma0=300.0,
                            theta_c=0.1, k_e=2.0, k_g=2.0, tau=1.0, E_iso_w=1e52, Gamma0_w=300.0,
                            theta_w=math.pi / 2, p=2.3, eps_e=0.1, eps_B=0.01, xi_e=1.0,
                            p_r=2.3, eps_e_r=0.1, eps_B_r=0.01, xi_e_r=1.0, L0=0.0, t0=1.0, q=2.0)

_dp = C.POINTER(C.c_double)


def _device_prior(prior):
    """(VAG_PRIOR_* kind, a, b) of a prior the device evaluates itself; PRIOR_NONE hands an unknown object's ln_prob to the host.
    Recognised by shape, not by import: bilby.core.prior.Uniform(minimum, maximum) (its own support: -ln(maximum - minimum)
    inside, -inf outside), Gaussian(mu, sigma), LogUniform(minimum, maximum), or tuples ("uniform",) = the ParamDef's own
    Uniform(lower, upper), ("uniform", lo, hi), ("gaussian", mu, sigma), ("log_uniform", lo, hi)."""
    if prior is None:
        return _lib.PRIOR_UNIFORM, 0.0, 0.0
    if isinstance(prior, (tuple, list)):
        name = str(prior[0]).lower()
        if name == "uniform":
            if len(prior) >= 3:
                return _lib.PRIOR_UNIFORM_RANGE, float(prior[1]), float(prior[2])
            return _lib.PRIOR_UNIFORM, 0.0, 0.0
        if name in ("gaussian", "normal"):
            return _lib.PRIOR_GAUSSIAN, float(prior[1]), float(prior[2])
        if name in ("log_uniform", "loguniform"):
            return _lib.PRIOR_LOG_UNIFORM, float(prior[1]), float(prior[2])
        raise ValueError(f"unknown prior {prior!r}")
    cls = type(prior).__name__
    if cls in ("Gaussian", "Normal") and hasattr(prior, "mu") and hasattr(prior, "sigma"):
        return _lib.PRIOR_GAUSSIAN, float(prior.mu), float(prior.sigma)
    if cls == "LogUniform" and hasattr(prior, "minimum") and hasattr(prior, "maximum"):
        return _lib.PRIOR_LOG_UNIFORM, float(prior.minimum), float(prior.maximum)
    if cls == "Uniform" and hasattr(prior, "minimum") and hasattr(prior, "maximum"):
        return _lib.PRIOR_UNIFORM_RANGE, float(prior.minimum), float(prior.maximum)
    if not hasattr(prior, "ln_prob"):
        raise ValueError(f"prior {prior!r} has no ln_prob")
    return _lib.PRIOR_NONE, 0.0, 0.0


def host_ln_prior(samples, lower, upper, prior_specs):
    """sum_d ln prior_d(samples[:, d]) with the bounds mask of fitting/samplers.py:72-91 on the host: -inf outside
    [lower, upper], else the closed forms of bilby's Uniform / Gaussian / LogUniform (the same expressions
    vag_fit_front_kernel evaluates) or the prior object's own ln_prob.  prior_specs[d] = (kind, a, b, obj)."""
    samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    lp = np.zeros(samples.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for d, (kind, a, b, obj) in enumerate(prior_specs):
            x = samples[:, d]
            if kind == _lib.PRIOR_UNIFORM:
                lp += -np.log(upper[d] - lower[d])
            elif kind == _lib.PRIOR_UNIFORM_RANGE:
                lp += np.where((x >= a) & (x <= b), -np.log(b - a), -np.inf)
            elif kind == _lib.PRIOR_GAUSSIAN:
                lp += -0.5 * ((x - a) / b) ** 2 - np.log(b * 2.5066282746310002)
            elif kind == _lib.PRIOR_LOG_UNIFORM:
                lp += np.where((x >= a) & (x <= b), -np.log(x * np.log(b / a)), -np.inf)
            else:
                lp += np.asarray(obj.ln_prob(x), dtype=np.float64)
    inside = np.all((samples >= lower) & (samples <= upper), axis=1)
    lp[~inside] = -np.inf
    lp[~np.isfinite(lp)] = -np.inf
    return lp


INDEX_CONVENTIONS = ("slope", "beta", "photon")


def index_coefficients(nu):
    """The least-squares coefficients of a spectral-index group: c_k = (x_k - mean x) / sum_j (x_j - mean x)^2 with x = ln nu, so
    that sum_k c_k ln F_k is the least-squares slope d ln F / d ln nu over the nodes (sum c = 0 and sum c x = 1 to rounding).  Two
    nodes: c = (-1, 1) / ln(nu_1 / nu_0)."""
    nu = np.asarray(nu, dtype=np.float64)
    x = np.log(nu / nu[0])  # (the shift by ln nu_0 changes no c_k; it keeps the rounding of ln nu ~ 40 out of the differences)
    if x.size == 2:
        return np.array([-1.0 / x[1], 1.0 / x[1]])
    dx = x - x.mean()
    return dx / np.sum(dx * dx)


def index_slope(F, coef):
    """S = sum_{k >= 1} c_k ln(F_k / F_0) along the last axis of F, summed in k order: the statement of the device's
    vag::log_slope (the pivot form: every log is taken of a ratio to F_0; c_0 is not read).  NaN where some F_k is <= 0 or not
    finite."""
    F = np.asarray(F, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    ok = np.all(np.isfinite(F) & (F > 0), axis=-1)
    s = np.zeros(F.shape[:-1])
    with np.errstate(all="ignore"):
        for k in range(1, F.shape[-1]):
            s = s + coef[k] * np.log(F[..., k] / F[..., 0])
    return np.where(ok, s, np.nan)


def index_from_slope(slope, convention):
    """A slope s (F_nu ~ nu^s) in the convention of the data: "slope" s, "beta" -s (F_nu ~ nu^-beta), "photon" 1 - s
    (N_E ~ E^-Gamma).  The map is its own inverse."""
    if convention == "slope":
        return +np.asarray(slope, dtype=np.float64)
    if convention == "beta":
        return -np.asarray(slope, dtype=np.float64)
    if convention == "photon":
        return 1.0 - np.asarray(slope, dtype=np.float64)
    raise ValueError(f"unknown spectral-index convention {convention!r}: one of {INDEX_CONVENTIONS}")


def _widest_entry(lib, spec, suffix):
    """The likelihood entry point that serves the spec, and its trailing spec arguments.  A fit with correlated groups goes through
    vag_loglike_cov_batch<suffix>; every other fit through the widest of vag_loglike_tmpl_batch<suffix> and
    vag_loglike_fold_batch<suffix> that the loaded library has, the call it always made.  All three were added after ABI 13 and are
    detected by symbol.  A library without the template entry (VAG_LIB_PATH naming an older build) serves every fit without templates
    through the fold entry, and one without that every fit without count spectra through vag_loglike_index_batch<suffix>, the same
    call bit for bit; a fit with correlated groups, templates or count spectra is an error where its entry is missing."""
    tmpl = getattr(spec, "_tmpl", None)
    cov = getattr(spec, "_cov", None)
    if getattr(spec, "_robust", None) is not None:
        # outlier groups: the request form.  The callers hand every entry (h, spec, the blocks ..., theta, nb, ndim, out); the blocks
        # travel in the request here, so the function handed back keeps the context and the four trailing arguments
        name = "vag_loglike_robust_batch" + suffix
        if not hasattr(lib, name):
            raise RuntimeError(f"the loaded library has no {name}: outlier groups (outliers=True of Fitter.add_flux_density / "
                               "add_spectrum / add_flux) need a newer build")
        entry, request = getattr(lib, name), loglike_request(spec)
        return (lambda h, *args: entry(h, C.byref(request), *args[-4:])), ()
    if cov is not None:
        name = "vag_loglike_cov_batch" + suffix
        if not hasattr(lib, name):
            raise RuntimeError(f"the loaded library has no {name}: correlated groups (Fitter.add_correlated) need a newer build")
        return getattr(lib, name), (C.byref(spec._fold) if spec._fold is not None else None, C.byref(tmpl) if tmpl is not None else None,
                                    C.byref(cov))
    name = "vag_loglike_tmpl_batch" + suffix
    if hasattr(lib, name):
        return getattr(lib, name), (C.byref(spec._fold) if spec._fold is not None else None, C.byref(tmpl) if tmpl is not None else None)
    if tmpl is not None:
        raise RuntimeError(f"the loaded library has no {name}: additive templates (templates=... of Fitter.add_flux_density / "
                           "add_spectrum / add_flux) need a newer build")
    name = "vag_loglike_fold_batch" + suffix
    if hasattr(lib, name):
        return getattr(lib, name), (C.byref(spec._fold) if spec._fold is not None else None,)
    if spec._fold is not None:
        raise RuntimeError(f"the loaded library has no {name}: count spectra (Fitter.add_count_spectrum) need a newer build")
    return getattr(lib, "vag_loglike_index_batch" + suffix), ()


def on_current_stream(lib, h, lock, dev, fn):
    """fn() with the context (h, lock) on torch's current stream of ``dev``: the context follows that stream for the duration of the
    call and then goes back to the stream it was on -- a stream the caller destroys later must not stay bound to the (shared)
    context."""
    import torch
    with lock:
        prev = C.c_void_p()
        _lib.check(lib.vag_ctx_get_stream(h, C.byref(prev)))
        _lib.check(lib.vag_ctx_set_stream(h, _lib.torch_stream_handle(torch.cuda.current_stream(dev))))
        try:
            return fn()
        finally:
            lib.vag_ctx_set_stream(h, prev)


def loglike_request(spec):
    """vag_loglike_request of a spec made by Fitter.build_spec: the twelve blocks of the widest likelihood entry, None where the fit
    has none.  The struct points into ``spec``: keep both."""
    ptr = lambda x: C.pointer(x) if x is not None else None  # noqa: E731
    return _lib.LoglikeRequest(C.pointer(spec), ptr(spec._sky), ptr(spec._vis), ptr(spec._pol), ptr(spec._lim), ptr(spec._noise),
                               ptr(spec._counts), ptr(spec._index), ptr(spec._fold), ptr(spec._tmpl), ptr(spec._cov),
                               ptr(getattr(spec, "_robust", None)))


def outlier_terms(r, sigma, w, s, frac, scale, shift):
    """(lnl, p_out) of the detection rows of one outlier group, the numpy statement of the device's term (INTEGRATION.md "Outlier
    groups"): r [..., n] the residuals ln F_obs - ln max(f, 1e-300), sigma [n] the rows' ln_err, w [n] their weights; s the group's
    systematic, frac its outlier fraction P in [0, 1), scale the extra scatter b >= 0 and shift the mean offset mu of outliers in ln F,
    each a scalar or [...] (one per walker).
        v_in = sigma^2 + s^2,  v_out = v_in + b^2,
        g = log1p(-P) - r^2 / (2 v_in)         - log1p(s^2 / sigma^2) / 2
        o = ln P      - (r - mu)^2 / (2 v_out) - log1p((s^2 + b^2) / sigma^2) / 2
        l = max(g, o) + log1p(exp(-|g - o|))
    lnl [...] = sum_i w_i l_i is what the rows add to ln L; p_out [..., n] = exp(o - l) is each row's posterior probability of being
    an outlier at these parameters.  ln 0 = -inf as it stands: P = 0 gives l = g, the noise group's term, and p_out = 0."""
    r, sig, w = np.asarray(r, dtype=np.float64), np.asarray(sigma, dtype=np.float64), np.asarray(w, dtype=np.float64)
    s2, P, b2, mu = (np.asarray(v, dtype=np.float64)[..., None] for v in (s, frac, scale, shift))
    s2, b2 = s2 * s2, b2 * b2
    sig2 = sig * sig
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = np.log1p(-P) - 0.5 * (r * r) / (sig2 + s2) - 0.5 * np.log1p(s2 / sig2)
        o = np.log(P) - 0.5 * ((r - mu) * (r - mu)) / (sig2 + s2 + b2) - 0.5 * np.log1p((s2 + b2) / sig2)
        hi = np.where(g > o, g, o)
        ell = hi + np.log1p(np.exp(-np.abs(g - o)))
        p_out = np.exp(o - ell)
        return np.sum(w * ell, axis=-1), p_out


def _fma(a, b, c):
    """a * b + c with one rounding, in numpy: the product split without error (Veltkamp / Dekker), the sum without error (Knuth), the
    two error terms added to the rounded sum.  For finite operands far from overflow and underflow, as template values are."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        p = a * b
        ta, tb = 134217729.0 * a, 134217729.0 * b
        ah, bh = ta - (ta - a), tb - (tb - b)
        al, bl = a - ah, b - bh
        ep = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s = p + c
        v = s - p
        es = (p - (s - v)) + (c - v)
        return np.where(np.isfinite(ep + es), s + (ep + es), s)


def template_terms(T, amp, extinguished):
    """(e, x) of the additive templates, the numpy statement of the device's term: T [n_templates, n] the templates' values at the
    rows, amp [..., n_templates] the amplitudes (one set per walker), extinguished [n_templates] flags;
        e[..., i] = sum_c amp[..., c] T[c, i] over the templates with extinguished = 0,
        x[..., i] = the same over the templates with extinguished = 1,
    both from 0 in ascending c with one fma per term (_fma: exact to a rounding).  A row's model value is then
    (F + x) exp(-A_V k) + e."""
    T = np.asarray(T, dtype=np.float64)
    amp = np.asarray(amp, dtype=np.float64)
    flags = np.asarray(extinguished).astype(bool).reshape(-1)
    if T.ndim != 2 or amp.shape[-1] != T.shape[0] or flags.size != T.shape[0]:
        raise ValueError(f"template_terms: T must be [n_templates, n] with one amplitude and one flag per template, got T {T.shape}, "
                         f"amp {amp.shape}, extinguished {flags.shape}")
    e = np.zeros(amp.shape[:-1] + (T.shape[1],))
    x = np.zeros_like(e)
    for c in range(T.shape[0]):
        if flags[c]:
            x = _fma(amp[..., c, None], T[c], x)
        else:
            e = _fma(amp[..., c, None], T[c], e)
    return e, x


def covariance_whitener(C):
    """The whitener W of a covariance C [n, n]: lower triangular with positive diagonal, W C W^T = I -- the inverse of C's Cholesky
    factor L, formed column by column by forward substitution.  C must be finite, symmetric (|C_ij - C_ji| <= 1e-12 sqrt(C_ii C_jj))
    and positive definite.  Raises ValueError("... too ill-conditioned") when max |W C W^T - I|, formed in numpy.longdouble, exceeds
    1e-6: the fitter's default rtol, beyond which the term is wrong at the level of the model itself."""
    C_ = np.asarray(C, dtype=np.float64)
    if C_.ndim != 2 or C_.shape[0] != C_.shape[1] or C_.shape[0] == 0:
        raise ValueError(f"covariance_whitener: the covariance must be [n, n] with n >= 1, got {C_.shape}")
    if not np.isfinite(C_).all():
        raise ValueError("covariance_whitener: the covariance must be finite")
    n = C_.shape[0]
    if n > _lib.COV_MAX_ROWS:
        raise ValueError(f"covariance_whitener: at most {_lib.COV_MAX_ROWS} rows per correlated group, got {n}")
    d = np.diag(C_)
    if (d <= 0).any():
        raise ValueError("covariance_whitener: the covariance is not positive definite (a diagonal entry is <= 0)")
    scale = np.sqrt(d[:, None] * d[None, :])
    if (np.abs(C_ - C_.T) > 1e-12 * scale).any():
        raise ValueError("covariance_whitener: the covariance is not symmetric (|C_ij - C_ji| > 1e-12 sqrt(C_ii C_jj))")
    try:
        L = np.linalg.cholesky(C_)
    except np.linalg.LinAlgError:
        raise ValueError("covariance_whitener: the covariance is not positive definite") from None
    W = np.zeros_like(C_)
    for k in range(n):  # column k of L^-1: forward substitution on the k-th unit vector
        for i in range(k, n):
            s = (1.0 if i == k else 0.0) - np.dot(L[i, k:i], W[k:i, k])
            W[i, k] = s / L[i, i]
    Wl, Cl = W.astype(np.longdouble), C_.astype(np.longdouble)
    resid = np.abs(Wl @ Cl @ Wl.T - np.eye(n, dtype=np.longdouble)).max()
    if not np.isfinite(W).all() or not resid <= 1e-6:
        raise ValueError(f"covariance_whitener: the covariance is too ill-conditioned (max |W C W^T - I| = {float(resid):.3g} > 1e-6)")
    return W


def whitened_chi2(r, W):
    """sum_i (sum_{j <= i} W_ij r_j)^2 along the last axis of r [..., n], W [n, n] lower triangular: the numpy statement of the
    device's correlated-group term.  Each y_i is summed from 0 in ascending j, then the squares in ascending i (the device forms y_i
    with one fma per term and closes lane-strided sums: the two agree to rounding)."""
    r = np.asarray(r, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    n = r.shape[-1]
    if W.shape != (n, n):
        raise ValueError(f"whitened_chi2: W must be [{n}, {n}], got {W.shape}")
    chi2 = np.zeros(r.shape[:-1])
    for i in range(n):
        y = np.zeros(r.shape[:-1])
        for j in range(i + 1):
            y = y + W[i, j] * r[..., j]
        chi2 = chi2 + y * y
    return chi2


def _poisson_const(N):
    """S(N) = N ln N - N - ln N! per entry (0 for N = 0), as vag::poisson_const forms it: Stirling's remainder series from N = 16 on
    (no difference of large numbers), the three-term difference below."""
    N = np.asarray(N, dtype=np.float64)
    big = N >= 16
    i = 1.0 / np.where(big, N, 1.0)
    i2 = i * i
    series = i * (1 / 12 + i2 * (-1 / 360 + i2 * (1 / 1260 + i2 * (-1 / 1680 + i2 * (1 / 1188 + i2 * (-691 / 360360))))))
    out = np.where(big, -(0.5 * np.log(2 * np.pi * np.where(big, N, 1.0)) + series), 0.0)
    small = (N > 0) & ~big
    if small.any():
        out[small] = [n * math.log(n) - n - math.lgamma(n + 1.0) for n in N[small]]
    return out


def fold_expected(F, group, n_h=0.0):
    """The expected counts mu [..., n, C] of a count-spectrum group (an entry of Fitter._fold_obs) on model flux densities
    F [..., n_samples * J] at the group's points (t_sample_s, nu_j), s outer -- the numpy statement of the fold term:
        G[i][j]  = T_j ((exposure_i / m) sum_s F[sample_idx[i][s]][j])   (summed in s order), T_j = exp(-N_H sigma_j) or 1,
        mu[i][c] = B[i][c] + sum_j A[j][c] G[i][j]                       (summed in ascending j from 0, B added last).
    n_h: a scalar or an array of the leading shape of F; not read by a group without absorption."""
    gd = group
    J, ns, n = gd["nu"].size, gd["t_sample"].size, gd["exposure_over_m"].size
    F = np.asarray(F, dtype=np.float64)
    if F.shape[-1] != ns * J:
        raise ValueError(f"fold_expected: F must hold n_samples * J = {ns * J} values along its last axis, got {F.shape}")
    F = F.reshape(F.shape[:-1] + (ns, J))
    with np.errstate(all="ignore"):
        total = np.zeros(F.shape[:-2] + (n, J))
        for k in range(gd["m"]):
            total = total + F[..., gd["sample_idx"][:, k], :]
        G = gd["exposure_over_m"][:, None] * total
        if gd["sigma"] is not None:
            T = np.exp(-(np.asarray(n_h, dtype=np.float64)[..., None] * gd["sigma"]))
            G = T[..., None, :] * G
        acc = np.zeros(F.shape[:-2] + (n, gd["A"].shape[1]))
        for j in range(J):
            acc = acc + gd["A"][j] * G[..., j, None]
        return gd["background"] + acc


class Fitter:
    """Fitter(*, z=0.0, lumi_dist=1e26, jet=..., medium=..., resolution=..., rtol=...): keyword-only with the reference's
    defaults (fitter.py:96-135)."""

    def __init__(self, *, z=0.0, lumi_dist=1e26, jet="tophat", medium="ism", resolution=None, rtol=1e-6,
                 radiative_fireball=True, device=0, fwd_ssc=False, kn=False, rvs_shock=False, rvs_ssc=False,
                 magnetar=False, extinction=None, n_h=0.0):
        # extinction: k(lambda_rest [cm]) -> A_lambda / A_V of the host-galaxy law (a callable; fitter.py:379-397).  The
        # point-data model fluxes are scaled by exp(-A_V * 0.4 ln10 * k) with A_V a (free or fixed) parameter.
        # A name selects a built-in Pei92 law; a custom callable is evaluated ONCE per data set (it must not depend on the
        # sampled parameters: the device likelihood applies one fixed kernel per datum).
        if isinstance(extinction, str):
            from .extinction import BUILTIN_LAWS
            if extinction not in BUILTIN_LAWS:
                raise ValueError(f"Unknown extinction law: {extinction!r}. Expected one of {sorted(BUILTIN_LAWS)} or a callable.")
            self.extinction_name, extinction = extinction, BUILTIN_LAWS[extinction]
        elif extinction is not None and not callable(extinction):
            raise ValueError("extinction must be None, 'smc' / 'lmc' / 'mw', or a callable k(lambda_rest_cm)")
        self.extinction = extinction
        # n_h: the absorbing column N_H [cm^-2] of the count-spectrum groups with absorption=... when N_H is not a parameter
        if not np.isfinite(n_h) or n_h < 0:
            raise ValueError(f"n_h must be finite and >= 0, got {n_h!r}")
        self.n_h = float(n_h)
        self.magnetar = bool(magnetar)
        if rvs_ssc and not rvs_shock:
            rvs_ssc = False  # the reference only builds rvs_rad when rvs_shock is on (fitter.py:476-484)
        self.fwd_ssc, self.kn, self.rvs_shock, self.rvs_ssc = bool(fwd_ssc), bool(kn), bool(rvs_shock), bool(rvs_ssc)
        if jet not in JET_TYPES:
            raise ValueError(f"Unknown jet type: {jet}")
        if medium not in MEDIUM_TYPES:
            raise ValueError(f"Unknown medium type: {medium}")
        self.z, self.lumi_dist, self.jet, self.medium = float(z), float(lumi_dist), jet, medium
        # None -> the Model ctor's mode-aware default (fitter.py:120-123, pymodel.h:630-637)
        if resolution is None:
            resolution = (0.06, 0.2, 10.0) if self.rvs_shock else (0.06, 0.15, 6.0)
        self.resolution, self.rtol, self.radiative_fireball = tuple(resolution), float(rtol), bool(radiative_fireball)
        self.device = device
        self._point_t, self._point_nu, self._point_flux, self._point_err, self._point_weights = [], [], [], [], []
        self._point_lim = []  # per add_* call: the boolean mask of its upper-limit rows (upper_limit=...)
        self._point_grp = []  # per add_* call: the noise group id of its rows (noise=...), -1 = none
        self._noise_labels = []  # the noise groups in order of first mention: group g is self._noise_labels[g]
        self._noise_calib = {}  # label -> its calibration fraction, once a call has stated one
        self._noise_robust = {}  # label -> its outliers= flag, once a call has stated one (robust: the mixture likelihood)
        self._point_tmpl = []  # per add_* call: {template id: its values at the call's rows} (templates=...)
        self._tmpl_names = []  # the templates in order of first mention: template c is self._tmpl_names[c]
        self._tmpl_ext = []  # per template: its extinguished flag (add_template)
        self._tmpl_used = set()  # the ids of the templates some row carries
        self._band_obs = []
        self._centroid_obs = []  # VLBI centroid groups (add_centroid): one vag_centroid_obs each
        self._vis_obs = []  # VLBI visibility groups (add_visibilities): one vag_visibility_obs each
        self._pol_obs = []  # polarization groups (add_polarization): one vag_polarization_obs each
        self._counts_obs = []  # photon-count groups (add_counts): one vag_counts_obs each
        self._index_obs = []  # spectral-index groups (add_spectral_index): one vag_index_obs each
        self._fold_obs = []  # count-spectrum groups (add_count_spectrum): one vag_fold_obs each
        self._cov_obs = []  # correlated groups (add_correlated): one vag_cov_obs each
        self._ext_kernel = None
        self._ext_kernels = {}  # z -> 0.4 ln10 k(lambda_rest) over the consolidated point data
        self._ext_z = float(z)
        self._all_t = None

    @staticmethod
    def _checked_observations(t, f_nu, err, weights, who):
        """The boundary checks of every add_* method (fitter.py:212-254): same shapes, non-empty, finite fluxes, finite
        positive errors, finite non-negative weights.  Returns float64 arrays (weights default to ones)."""
        t, f_nu, err = (np.asarray(a, dtype=np.float64) for a in (t, f_nu, err))
        if t.size == 0:
            raise ValueError(f"{who}: time array is empty")
        if not (t.shape == f_nu.shape == err.shape):
            raise ValueError(f"{who}: t, f_nu, err must have the same shape; got t.shape={t.shape}, "
                             f"f_nu.shape={f_nu.shape}, err.shape={err.shape}")
        if not np.isfinite(f_nu).all():
            raise ValueError(f"{who}: f_nu contains {int((~np.isfinite(f_nu)).sum())} non-finite (NaN or inf) values")
        if not np.isfinite(err).all() or (err <= 0).any():
            raise ValueError(f"{who}: err must be finite and > 0 at every point (got min={float(err.min())}, "
                             f"max={float(err.max())})")
        if weights is None:
            w = np.ones_like(t)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t.shape:
                raise ValueError(f"{who}: weights.shape={w.shape} must match t.shape={t.shape}")
            if not np.isfinite(w).all() or (w < 0).any():
                raise ValueError(f"{who}: weights must be finite and >= 0 at every point")
        return t, f_nu, err, w

    @staticmethod
    def _limit_mask(upper_limit, t, values, who):
        """The boolean mask of the rows that are upper limits: ``upper_limit`` is None / a bool (no / every row) or a boolean
        array of the shape of t.  On a flagged row the flux argument is the limit L >= 0 and the error argument the noise level
        sigma: the row adds -2 w ln Phi((L - model) / sigma) to chi^2 ("a 3 sigma limit of X" is L = X, sigma = X / 3)."""
        if upper_limit is None:
            return np.zeros(t.shape, dtype=bool)
        m = np.asarray(upper_limit)
        if m.dtype != np.bool_:
            raise ValueError(f"{who}: upper_limit must be a bool or a boolean mask, got dtype {m.dtype}")
        if m.ndim == 0:
            m = np.full(t.shape, bool(m))
        elif m.shape != t.shape:
            raise ValueError(f"{who}: an upper_limit mask must have the shape of t, got {m.shape} vs {t.shape}")
        if (values[m] < 0).any():
            raise ValueError(f"{who}: an upper limit must be >= 0")
        return m.copy()

    def _noise_group(self, noise, calibration, who, outliers=None):
        """The id of the noise group ``noise`` names (-1 for None), declared at its first mention.  noise: a label matching
        [A-Za-z0-9_]+; the rows join the group whose fractional systematic is the parameter ``sys_<label>`` (free or fixed; 0 when
        not given), added in quadrature to each row's relative error with the Gaussian normalisation.  calibration: the fraction
        c >= 0 by which the group's common flux scale is uncertain (a Gaussian prior on ln scale, marginalised); every call that
        states it for a label must state the same value.  outliers: True makes the group robust -- each of its detection rows is an
        inlier with probability 1 - P and is otherwise drawn from a broader, shifted Gaussian in ln F (the mixture of Hogg, Bovy &
        Lang 2010; parameters ``out_frac_<label>``, ``out_scale_<label>``, ``out_shift_<label>``); every call that states it for a
        label must state the same value, and a robust group takes no calibration.  At most 8 groups.  Nothing is recorded when the
        call raises."""
        if outliers is not None and not isinstance(outliers, (bool, np.bool_)):
            raise ValueError(f"{who}: outliers must be a bool, got {outliers!r}")
        if noise is None:
            if calibration is not None:
                raise ValueError(f"{who}: calibration needs noise=<label> (it is the calibration of a noise group)")
            if outliers:
                raise ValueError(f"{who}: outliers needs noise=<label> (a robust group is a noise group)")
            return -1
        if not isinstance(noise, str) or not re.fullmatch(r"[A-Za-z0-9_]+", noise):
            raise ValueError(f"{who}: noise must be a label matching [A-Za-z0-9_]+, got {noise!r}")
        if calibration is not None:
            try:
                calibration = float(calibration)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: calibration must be a number >= 0, got {calibration!r}") from None
            if not np.isfinite(calibration) or calibration < 0:
                raise ValueError(f"{who}: calibration must be finite and >= 0, got {calibration!r}")
            if self._noise_calib.get(noise, calibration) != calibration:
                raise ValueError(f"{who}: noise group {noise!r} has calibration={self._noise_calib[noise]!r} from an earlier call, "
                                 f"got {calibration!r}")
        if outliers is not None:
            outliers = bool(outliers)
            if self._noise_robust.get(noise, outliers) != outliers:
                raise ValueError(f"{who}: noise group {noise!r} has outliers={self._noise_robust[noise]!r} from an earlier call, "
                                 f"got {outliers!r}")
        robust = self._noise_robust.get(noise, False) if outliers is None else outliers
        if robust and (self._noise_calib.get(noise, 0.0) if calibration is None else calibration) > 0:
            raise ValueError(f"{who}: noise group {noise!r} cannot have both outliers=True and a calibration fraction: the marginalised "
                             "scale does not commute with the mixture")
        if noise not in self._noise_labels and len(self._noise_labels) >= _lib.NOISE_MAX_GROUPS:
            raise ValueError(f"{who}: at most {_lib.NOISE_MAX_GROUPS} noise groups, {noise!r} would be one more")
        if noise not in self._noise_labels:
            self._noise_labels.append(noise)
        if calibration is not None:
            self._noise_calib[noise] = calibration
        if outliers is not None:
            self._noise_robust[noise] = outliers
        return self._noise_labels.index(noise)

    def _checked_templates(self, templates, shape, who):
        """{name: float64 array of ``shape``} of a templates= argument, checked and with nothing recorded: a dict of names matching
        [A-Za-z0-9_]+ to a scalar or an array of the shape of the rows, finite and >= 0; at most 8 templates per fit."""
        if templates is None:
            return {}
        if not isinstance(templates, dict):
            raise ValueError(f"{who}: templates must be a dict {{name: values}}, got {type(templates).__name__}")
        out = {}
        for name, values in templates.items():
            if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z0-9_]+", name):
                raise ValueError(f"{who}: a template name must match [A-Za-z0-9_]+, got {name!r}")
            try:
                v = np.asarray(values, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: the values of template {name!r} must be numbers") from None
            if v.ndim != 0 and v.shape != shape:
                raise ValueError(f"{who}: the values of template {name!r} must be a scalar or have the shape of the rows {shape}, "
                                 f"got {v.shape}")
            if not np.isfinite(v).all() or (v < 0).any():
                raise ValueError(f"{who}: the values of template {name!r} must be finite and >= 0")
            out[name] = np.full(shape, float(v)) if v.ndim == 0 else v.copy()
        new = [name for name in out if name not in self._tmpl_names]
        if len(self._tmpl_names) + len(new) > _lib.TMPL_MAX:
            raise ValueError(f"{who}: at most {_lib.TMPL_MAX} templates, {new[_lib.TMPL_MAX - len(self._tmpl_names)]!r} would be one more")
        return out

    def _record_templates(self, checked):
        """{template id: values} of what _checked_templates returned; new names are declared plain, in order of mention."""
        out = {}
        for name, v in checked.items():
            if name not in self._tmpl_names:
                self._tmpl_names.append(name)
                self._tmpl_ext.append(False)
            c = self._tmpl_names.index(name)
            self._tmpl_used.add(c)
            out[c] = v
        return out

    def add_template(self, name, extinguished=False):
        """Declares the additive template ``name`` ahead of its first mention in a templates= argument -- the only way to set its
        flag.  extinguished=True: the template's light passes the host's dust like the afterglow's (a supernova, a kilonova); False:
        it does not (a host galaxy measured as it is seen).  A row's model value is (F + x) exp(-A_V k) + e with x / e the sums of
        amplitude * value over the extinguished / plain templates; the amplitude is the parameter ``amp_<name>`` (free on linear
        scale with lower >= 0, on log scale with lower > 0, or fixed >= 0; 0 when not given).  At most 8 templates per fit; the
        flag cannot change once rows carry the template."""
        if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z0-9_]+", name):
            raise ValueError(f"add_template: a template name must match [A-Za-z0-9_]+, got {name!r}")
        if not isinstance(extinguished, (bool, np.bool_)):
            raise ValueError(f"add_template: extinguished must be a bool, got {extinguished!r}")
        if name in self._tmpl_names:
            c = self._tmpl_names.index(name)
            if c in self._tmpl_used and self._tmpl_ext[c] != bool(extinguished):
                raise ValueError(f"add_template: rows already carry template {name!r} with extinguished={self._tmpl_ext[c]}: declare "
                                 "it before its first mention")
            self._tmpl_ext[c] = bool(extinguished)
            return
        if len(self._tmpl_names) >= _lib.TMPL_MAX:
            raise ValueError(f"add_template: at most {_lib.TMPL_MAX} templates, {name!r} would be one more")
        self._tmpl_names.append(name)
        self._tmpl_ext.append(bool(extinguished))

    def _add_points(self, t, nu, f_nu, err, w, lim, grp=-1, tmpl=None):
        self._point_tmpl.append(tmpl or {})
        self._point_lim.append(lim)
        self._point_grp.append(np.full(t.shape, grp, dtype=np.int32))
        self._point_t.append(t)
        self._point_nu.append(nu)
        self._point_flux.append(f_nu)
        self._point_err.append(err)
        self._point_weights.append(w)
        self._all_t = None

    # fitter.py:256-282
    def add_flux_density(self, nu, t, f_nu, err, weights=None, label=None, upper_limit=None, noise=None, calibration=None,
                         templates=None, outliers=None):
        """Light-curve data at one frequency nu [Hz] (`label` is accepted for API compatibility; it only names plot legends).
        upper_limit: None, a bool or a boolean mask of the shape of t; on a flagged row f_nu is the limit L and err the noise level
        sigma (Fitter._limit_mask).  noise, calibration, outliers: the noise group of the rows, its calibration fraction and whether
        it is robust (Fitter._noise_group).  templates: {name: values} of the additive templates at these rows, values a scalar or an array of the
        shape of t in the unit of f_nu (Fitter.add_template); a host galaxy: templates={"host_r": 1.0} with the parameter
        amp_host_r."""
        nu_arr = np.asarray(nu, dtype=np.float64)
        if not np.isfinite(nu_arr).all() or (nu_arr <= 0).any():
            raise ValueError(f"add_flux_density: nu must be finite and > 0, got {nu}")
        t, f_nu, err, w = self._checked_observations(t, f_nu, err, weights, "add_flux_density")
        if nu_arr.ndim != 0 and nu_arr.shape != t.shape:  # extension: one frequency per point
            raise ValueError(f"add_flux_density: an array nu must have the shape of t, got {nu_arr.shape} vs {t.shape}")
        lim = self._limit_mask(upper_limit, t, f_nu, "add_flux_density")
        tmpl = self._checked_templates(templates, t.shape, "add_flux_density")
        grp = self._noise_group(noise, calibration, "add_flux_density", outliers)
        self._add_points(t, np.full_like(t, float(nu_arr)) if nu_arr.ndim == 0 else nu_arr.copy(), f_nu, err, w, lim, grp,
                         self._record_templates(tmpl))

    # fitter.py:284-314
    def add_spectrum(self, t, nu, f_nu, err, weights=None, upper_limit=None, noise=None, calibration=None, templates=None,
                     outliers=None):
        """A broadband spectrum at one time t [s]: one point-data row per frequency.  upper_limit: None, a bool or a boolean mask of
        the shape of nu; on a flagged row f_nu is the limit L and err the noise level sigma (Fitter._limit_mask).  noise, calibration,
        outliers: the noise group of the rows, its calibration fraction and whether it is robust (Fitter._noise_group).  templates: {name: values} of the additive
        templates at these rows, values a scalar or an array of the shape of nu (Fitter.add_template)."""
        if np.ndim(t) != 0 or not np.isfinite(t) or t <= 0:
            raise ValueError(f"add_spectrum: t must be finite and > 0, got {t}")
        nu = np.asarray(nu, dtype=np.float64)
        if nu.size and (not np.isfinite(nu).all() or (nu <= 0).any()):
            raise ValueError(f"add_spectrum: nu must be finite and > 0 at every point (got min={float(nu.min())}, "
                             f"max={float(nu.max())})")
        nu, f_nu, err, w = self._checked_observations(nu, f_nu, err, weights, "add_spectrum")  # nu is the axis array here
        lim = self._limit_mask(upper_limit, nu, f_nu, "add_spectrum")
        tmpl = self._checked_templates(templates, nu.shape, "add_spectrum")
        grp = self._noise_group(noise, calibration, "add_spectrum", outliers)
        self._add_points(np.full_like(nu, float(t)), nu, f_nu, err, w, lim, grp, self._record_templates(tmpl))

    # fitter.py:316-377
    def add_flux(self, band, t, flux, err, num_points=5, weights=None, upper_limit=None, noise=None, calibration=None,
                 templates=None, outliers=None):
        """Band-integrated fluxes [erg/cm^2/s] over band = (nu_min, nu_max) [Hz]; each group is one Model.flux request.
        upper_limit: None, a bool or a boolean mask of the shape of t; on a flagged row flux is the limit L >= 0 and err the noise
        level sigma (Fitter._limit_mask); detections need strictly positive fluxes.  noise, calibration: the noise group of the rows
        and its calibration fraction (Fitter._noise_group); a group with calibration > 0 holds point rows only or exactly one
        add_flux call (build_spec checks it); outliers: whether the group is robust (Fitter._noise_group).  templates: {name: values} of the additive templates at these rows, values a scalar or
        an array of the shape of t in erg/cm^2/s (Fitter.add_template)."""
        try:
            nu_min, nu_max = band
        except (TypeError, ValueError):
            raise ValueError(f"add_flux: band must be a (nu_min, nu_max) tuple in Hz, got {band!r}") from None
        if not (np.isfinite(nu_min) and np.isfinite(nu_max) and 0 < nu_min < nu_max):
            raise ValueError(f"add_flux: band must satisfy 0 < nu_min < nu_max with both finite; got nu_min={nu_min}, "
                             f"nu_max={nu_max}")
        if num_points < 2:
            raise ValueError(f"add_flux: num_points must be >= 2 for band integration, got {num_points}")
        t, flux, err, w = self._checked_observations(t, flux, err, weights, "add_flux")
        if t.ndim != 1:
            raise ValueError("add_flux: t, flux and err must be 1-D arrays")
        lim = self._limit_mask(upper_limit, t, flux, "add_flux")
        if np.any(flux[~lim] <= 0):
            raise ValueError("add_flux: the log-flux likelihood requires strictly positive fluxes")
        tmpl = self._checked_templates(templates, t.shape, "add_flux")
        order = np.argsort(t)
        bd = dict(nu_min=float(nu_min), nu_max=float(nu_max), num_points=int(num_points),
                  t=np.ascontiguousarray(t[order]), weights=np.ascontiguousarray(w[order]), lim=None,
                  noise=self._noise_group(noise, calibration, "add_flux", outliers))
        bd["tmpl"] = {c: np.ascontiguousarray(v[order]) for c, v in self._record_templates(tmpl).items()}  # the values follow the sort
        if lim.any():  # limit rows: ln_flux / ln_err are not read there (0 and 1); L and sigma go into their own arrays
            lim, flux, err = lim[order], flux[order], err[order]
            safe = np.where(lim, 1.0, flux)
            bd.update(ln_flux=np.ascontiguousarray(np.where(lim, 0.0, np.log(safe))),
                      ln_err=np.ascontiguousarray(np.where(lim, 1.0, err / safe)), lim=np.ascontiguousarray(lim, dtype=np.int32),
                      limit=np.ascontiguousarray(np.where(lim, flux, 0.0)), sigma=np.ascontiguousarray(np.where(lim, err, 1.0)))
        else:
            bd.update(ln_flux=np.ascontiguousarray(np.log(flux[order])), ln_err=np.ascontiguousarray(err[order] / flux[order]))
        self._band_obs.append(bd)

    def add_counts(self, band, t_start, exposure, counts, conversion, background=0.0, num_points=5, num_exposure_points=1,
                   weights=None):
        """Photon counts with a Poisson likelihood (the Cash statistic): row i observed counts[i] photons in band = (nu_min, nu_max)
        [Hz] during [t_start[i], t_start[i] + exposure[i]] [s].  The expected counts are
            mu_i = background_i + conversion_i * exposure_i * <F>_i,
        conversion [counts per erg cm^-2] (effective area over mean photon energy; a scalar or one per row), background [counts]
        (a scalar or one per row, >= 0), <F>_i the model's band-integrated flux (Model.flux with num_points Boole nodes) averaged
        over the window: num_exposure_points = 1 takes the midpoint t_start + exposure / 2, m >= 2 the mean of the m equally spaced
        samples t_start + k exposure / (m - 1), k = 0 .. m-1 (both ends, as Model.flux_density_exposures).  The row adds
        w_i [N_i ln mu_i - mu_i - ln N_i!] to ln L; N_i = 0 is a valid row (a non-detection).  The samples of all rows are merged into
        one strictly ascending list, equal times evaluated once, so contiguous bins share their end points; the group is one
        Model.flux request on that list.  Weights are used as given.  Nothing is recorded when the call raises."""
        who = "add_counts"
        try:
            nu_min, nu_max = band
        except (TypeError, ValueError):
            raise ValueError(f"{who}: band must be a (nu_min, nu_max) tuple in Hz, got {band!r}") from None
        if not (np.isfinite(nu_min) and np.isfinite(nu_max) and 0 < nu_min < nu_max):
            raise ValueError(f"{who}: band must satisfy 0 < nu_min < nu_max with both finite; got nu_min={nu_min}, nu_max={nu_max}")
        if int(num_points) != num_points or num_points < 2:
            raise ValueError(f"{who}: num_points must be an integer >= 2 for band integration, got {num_points!r}")
        if int(num_exposure_points) != num_exposure_points or num_exposure_points < 1:
            raise ValueError(f"{who}: num_exposure_points must be an integer >= 1, got {num_exposure_points!r}")
        m = int(num_exposure_points)
        t0, expo, N = (np.asarray(a, dtype=np.float64) for a in (t_start, exposure, counts))
        if t0.ndim != 1 or t0.size == 0:
            raise ValueError(f"{who}: t_start must be a non-empty 1-D array")
        if not (t0.shape == expo.shape == N.shape):
            raise ValueError(f"{who}: t_start, exposure and counts must have the same shape; got {t0.shape}, {expo.shape}, {N.shape}")
        if not np.isfinite(t0).all() or (t0 <= 0).any():
            raise ValueError(f"{who}: t_start must be finite and > 0 at every row")
        if not np.isfinite(expo).all() or (expo <= 0).any():
            raise ValueError(f"{who}: exposure must be finite and > 0 at every row")
        if not np.isfinite(N).all() or (N < 0).any() or (N != np.floor(N)).any():
            raise ValueError(f"{who}: counts must be finite integers >= 0")
        if (N > 2.0 ** 53).any():
            raise ValueError(f"{who}: counts above 2^53 are not supported")

        def per_row(value, name):
            a = np.asarray(value, dtype=np.float64)
            if a.ndim != 0 and a.shape != t0.shape:
                raise ValueError(f"{who}: {name} must be a scalar or have the shape of t_start, got {a.shape} vs {t0.shape}")
            return np.broadcast_to(a, t0.shape).copy()
        conv, bkg = per_row(conversion, "conversion"), per_row(background, "background")
        if not np.isfinite(conv).all() or (conv <= 0).any():
            raise ValueError(f"{who}: conversion must be finite and > 0 at every row")
        if not np.isfinite(bkg).all() or (bkg < 0).any():
            raise ValueError(f"{who}: background must be finite and >= 0 at every row")
        if weights is None:
            w = np.ones_like(t0)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t0.shape or not np.isfinite(w).all() or (w < 0).any():
                raise ValueError(f"{who}: weights must have the shape of t_start and be finite and >= 0")
        if m == 1:
            times = (t0 + 0.5 * expo)[:, None]
        else:
            times = t0[:, None] + np.arange(m, dtype=np.float64)[None, :] * (expo / float(m - 1))[:, None]
        if not np.isfinite(times).all():
            raise ValueError(f"{who}: t_start + exposure must be finite")
        t_sample, inverse = np.unique(times.ravel(), return_inverse=True)  # ascending, equal times once
        with np.errstate(over="ignore"):
            scale = conv * expo / float(m)
        if not np.isfinite(scale).all() or (scale <= 0).any():
            raise ValueError(f"{who}: conversion * exposure must be finite and > 0 at every row")
        c = np.ascontiguousarray
        self._counts_obs.append(dict(nu_min=float(nu_min), nu_max=float(nu_max), num_points=int(num_points), m=m,
                                     t_sample=c(t_sample), sample_idx=c(inverse.reshape(t0.size, m), dtype=np.int32), counts=c(N),
                                     background=c(bkg), scale=c(scale), weights=c(w)))

    @property
    def has_counts(self):
        """Some data are photon counts (add_counts)."""
        return bool(self._counts_obs)

    def add_spectral_index(self, band, t, index, err, num_points=2, convention="slope", weights=None):
        """Measured spectral indices over band = (nu_min, nu_max) [Hz] at times t [s]: a photon index per X-ray epoch, an optical
        slope per night.  The model's index is the least-squares slope d ln F_nu / d ln nu of the flux density over num_points
        (2..8) nodes, logspace(nu_min, nu_max) with the last node exactly nu_max; two nodes give ln(F_1 / F_0) / ln(nu_1 / nu_0).
        convention: "slope" (F_nu ~ nu^index), "beta" (F_nu ~ nu^-index) or "photon" (N_E ~ E^-index, slope = 1 - index); err is
        the error of the index in any of them.  A row adds w ((S - s) / err)^2 to chi^2; with Fitter(extinction=...) the model
        slope carries the law's reddening over the nodes times the walker's A_V.  A walker whose flux is not positive at some node
        of a row with w > 0 scores -inf.  Weights are used as given; rows are sorted by t.  Nothing is recorded when the call
        raises."""
        who = "add_spectral_index"
        try:
            nu_min, nu_max = band
        except (TypeError, ValueError):
            raise ValueError(f"{who}: band must be a (nu_min, nu_max) tuple in Hz, got {band!r}") from None
        if not (np.isfinite(nu_min) and np.isfinite(nu_max) and 0 < nu_min < nu_max):
            raise ValueError(f"{who}: band must satisfy 0 < nu_min < nu_max with both finite; got nu_min={nu_min}, nu_max={nu_max}")
        if int(num_points) != num_points or not (2 <= num_points <= _lib.INDEX_MAX_NODES):
            raise ValueError(f"{who}: num_points must be an integer in 2..{_lib.INDEX_MAX_NODES}, got {num_points!r}")
        if convention not in INDEX_CONVENTIONS:
            raise ValueError(f"{who}: unknown convention {convention!r}: one of {INDEX_CONVENTIONS}")
        t, idx, err = (np.asarray(a, dtype=np.float64) for a in (t, index, err))
        if t.ndim != 1 or t.size == 0:
            raise ValueError(f"{who}: t must be a non-empty 1-D array")
        if not (t.shape == idx.shape == err.shape):
            raise ValueError(f"{who}: t, index and err must have the same shape; got {t.shape}, {idx.shape}, {err.shape}")
        if not np.isfinite(t).all() or (t <= 0).any():
            raise ValueError(f"{who}: t must be finite and > 0 at every row")
        if not np.isfinite(idx).all():
            raise ValueError(f"{who}: index must be finite at every row")
        if not np.isfinite(err).all() or (err <= 0).any():
            raise ValueError(f"{who}: err must be finite and > 0 at every row")
        if weights is None:
            w = np.ones_like(t)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t.shape or not np.isfinite(w).all() or (w < 0).any():
                raise ValueError(f"{who}: weights must have the shape of t and be finite and >= 0")
        nu = np.logspace(np.log10(float(nu_min)), np.log10(float(nu_max)), int(num_points))
        nu[-1] = float(nu_max)
        if not (np.isfinite(nu).all() and (np.diff(nu) > 0).all()):
            raise ValueError(f"{who}: the band is too narrow for {num_points} distinct nodes; got nu_min={nu_min}, nu_max={nu_max}")
        coef = index_coefficients(nu)
        if not np.isfinite(coef).all():
            raise ValueError(f"{who}: the band is too narrow for finite slope coefficients; got nu_min={nu_min}, nu_max={nu_max}")
        order = np.argsort(t, kind="stable")
        c = np.ascontiguousarray
        self._index_obs.append(dict(nu=c(nu), coef=c(coef), convention=convention, t=c(t[order]),
                                    value=c(index_from_slope(idx[order], convention)), err=c(err[order]), weights=c(w[order])))

    @property
    def has_spectral_indices(self):
        """Some data are spectral indices (add_spectral_index)."""
        return bool(self._index_obs)

    def add_correlated(self, nu, t, f_nu, cov, weight=1.0):
        """Flux densities f_nu at times t [s] and frequency nu [Hz] (a scalar or an array of the shape of t) whose errors are
        correlated: cov [n, n] is their covariance in the unit of f_nu squared, 1 <= n <= 256; a fit holds at most 8 such groups.
        The group adds weight * r^T C_ln^-1 r to chi^2, r_i = ln f_nu,i - ln F_model,i (with the host's extinction as on the point
        rows) and C_ln,ij = cov_ij / (f_i f_j) the covariance of the log fluxes; the walker-independent ln det C_ln is not added.
        The rows are sorted by t (a stable sort), C_ln is permuted with them and then factored (covariance_whitener).  Recipes --
        a zero point shared by the rows, known to a fraction c:  cov = np.diag(err**2) + c**2 * np.outer(f_nu, f_nu);
        interstellar scintillation with modulation index m, a kernel in ln t and ln nu:
            cov = np.diag(err**2) + m**2 * np.outer(f_nu, f_nu) * np.exp(-0.5 * ((np.subtract.outer(np.log(t), np.log(t)) / l_t)**2
                                                                             + (np.subtract.outer(np.log(nu), np.log(nu)) / l_nu)**2)).
        Not supported inside a group: a free jitter or systematic, upper limits, templates, band-integrated rows; groups are
        independent of each other and of every other row.  Nothing is recorded when the call raises."""
        who = "add_correlated"
        nu_arr = np.asarray(nu, dtype=np.float64)
        t, f = np.asarray(t, dtype=np.float64), np.asarray(f_nu, dtype=np.float64)
        if t.ndim != 1 or t.size == 0:
            raise ValueError(f"{who}: t must be a non-empty 1-D array")
        n = t.size
        if n > _lib.COV_MAX_ROWS:
            raise ValueError(f"{who}: at most {_lib.COV_MAX_ROWS} rows per correlated group, got {n}")
        if f.shape != t.shape:
            raise ValueError(f"{who}: t and f_nu must have the same shape; got {t.shape}, {f.shape}")
        if nu_arr.ndim != 0 and nu_arr.shape != t.shape:
            raise ValueError(f"{who}: an array nu must have the shape of t, got {nu_arr.shape} vs {t.shape}")
        if not np.isfinite(nu_arr).all() or (nu_arr <= 0).any():
            raise ValueError(f"{who}: nu must be finite and > 0")
        if not np.isfinite(t).all() or (t <= 0).any():
            raise ValueError(f"{who}: t must be finite and > 0 at every row")
        if not np.isfinite(f).all() or (f <= 0).any():
            raise ValueError(f"{who}: f_nu must be finite and > 0 at every row (the likelihood is in ln f_nu)")
        cov = np.asarray(cov, dtype=np.float64)
        if cov.shape != (n, n):
            raise ValueError(f"{who}: cov must be [{n}, {n}], got {cov.shape}")
        if np.ndim(weight) != 0 or not np.isfinite(weight) or weight < 0:
            raise ValueError(f"{who}: weight must be a finite scalar >= 0, got {weight!r}")
        if len(self._cov_obs) >= _lib.COV_MAX_GROUPS:
            raise ValueError(f"{who}: at most {_lib.COV_MAX_GROUPS} correlated groups per fit")
        order = np.argsort(t, kind="stable")
        t, f = t[order], f[order]
        nu_rows = np.full_like(t, float(nu_arr)) if nu_arr.ndim == 0 else nu_arr[order]
        with np.errstate(all="ignore"):
            c_ln = cov[np.ix_(order, order)] / (f[:, None] * f[None, :])
        try:
            W = covariance_whitener(c_ln)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        c = np.ascontiguousarray
        self._cov_obs.append(dict(t=c(t), nu=c(nu_rows), ln_flux=c(np.log(f)), whitener=c(W), weight=float(weight)))

    @property
    def has_correlated(self):
        """Some data are correlated groups (add_correlated)."""
        return bool(self._cov_obs)

    def add_count_spectrum(self, energy_lo, energy_hi, response, t_start, exposure, counts, background=0.0, num_exposure_points=1,
                           weights=None, absorption=None):
        """Counts per detector channel of n spectra, compared with the model photon spectrum folded through the instrument
        response -- a Poisson likelihood (the Cash statistic) per row and channel.
        energy_lo, energy_hi [J]: the energy bins [keV, observer frame], 0 < lo < hi, ascending and non-overlapping (gaps are
        allowed), J <= 64.  response [C][J] >= 0 [cm^2]: counts in channel c per photon cm^-2 arriving in bin j (effective area x
        redistribution, rebinned to these bins, any fixed Galactic absorption folded in), C <= 256.  Row i observed counts[i][c] during
        [t_start[i], t_start[i] + exposure[i]] [s]; background [counts] and weights broadcast from a scalar, [C] or [n][C]; a weight of
        0 ignores a channel.  absorption [J]: a cross-section sigma_j >= 0 [cm^2 per H atom] at each bin, as the caller's table gives
        it for the absorber's redshift; the model is then multiplied by exp(-N_H sigma_j), N_H [cm^-2] the parameter "N_H" (free,
        fixed, or Fitter(n_h=...)), one N_H for all groups with absorption.  The expected counts are
            mu[i][c] = background[i][c] + sum_j A[j][c] T_j (exposure_i / m) sum_s F_nu(t_s, nu_j),
        nu_j = sqrt(lo_j hi_j) keV / h, A[j][c] = response[c][j] ln(hi_j / lo_j) / h (the midpoint rule in ln E of the photon
        spectrum over the bin), the m = num_exposure_points samples of a window and the merged sample list as in add_counts.  The
        term adds w [N ln mu - mu - ln N!] to ln L.  Each group is one flux-density request at its n_samples J points.  Nothing is
        recorded when the call raises."""
        who = "add_count_spectrum"
        from . import units
        lo, hi = (np.asarray(a, dtype=np.float64) for a in (energy_lo, energy_hi))
        if lo.ndim != 1 or lo.size == 0 or lo.shape != hi.shape:
            raise ValueError(f"{who}: energy_lo and energy_hi must be non-empty 1-D arrays of one shape; got {lo.shape}, {hi.shape}")
        if lo.size > _lib.FOLD_MAX_BINS:
            raise ValueError(f"{who}: energy_lo holds {lo.size} bins, at most {_lib.FOLD_MAX_BINS} are supported")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo <= 0).any() or (hi <= lo).any():
            raise ValueError(f"{who}: energy_lo and energy_hi must be finite with 0 < energy_lo < energy_hi in every bin")
        if (lo[1:] < hi[:-1]).any():
            raise ValueError(f"{who}: the bins of energy_lo / energy_hi must be ascending and must not overlap")
        J = lo.size
        R = np.asarray(response, dtype=np.float64)
        if R.ndim != 2 or R.shape[1] != J or R.shape[0] == 0:
            raise ValueError(f"{who}: response must be [channels][{J} bins], got {R.shape}")
        if R.shape[0] > _lib.FOLD_MAX_CHANNELS:
            raise ValueError(f"{who}: response holds {R.shape[0]} channels, at most {_lib.FOLD_MAX_CHANNELS} are supported")
        if not np.isfinite(R).all() or (R < 0).any():
            raise ValueError(f"{who}: response must be finite and >= 0")
        nC = R.shape[0]
        if int(num_exposure_points) != num_exposure_points or num_exposure_points < 1:
            raise ValueError(f"{who}: num_exposure_points must be an integer >= 1, got {num_exposure_points!r}")
        m = int(num_exposure_points)
        t0, expo, N = (np.asarray(a, dtype=np.float64) for a in (t_start, exposure, counts))
        if t0.ndim != 1 or t0.size == 0:
            raise ValueError(f"{who}: t_start must be a non-empty 1-D array")
        if expo.shape != t0.shape:
            raise ValueError(f"{who}: t_start and exposure must have the same shape; got {t0.shape}, {expo.shape}")
        if N.shape != (t0.size, nC):
            raise ValueError(f"{who}: counts must be [{t0.size} rows][{nC} channels], got {N.shape}")
        if not np.isfinite(t0).all() or (t0 <= 0).any():
            raise ValueError(f"{who}: t_start must be finite and > 0 at every row")
        if not np.isfinite(expo).all() or (expo <= 0).any():
            raise ValueError(f"{who}: exposure must be finite and > 0 at every row")
        if not np.isfinite(N).all() or (N < 0).any() or (N != np.floor(N)).any():
            raise ValueError(f"{who}: counts must be finite integers >= 0")
        if (N > 2.0 ** 53).any():
            raise ValueError(f"{who}: counts above 2^53 are not supported")

        def per_channel(value, name):
            a = np.asarray(value, dtype=np.float64)
            if a.ndim != 0 and a.shape != (nC,) and a.shape != N.shape:
                raise ValueError(f"{who}: {name} must be a scalar, [{nC} channels] or [{t0.size} rows][{nC} channels], got {a.shape}")
            return np.broadcast_to(a, N.shape).copy()
        bkg = per_channel(background, "background")
        if not np.isfinite(bkg).all() or (bkg < 0).any():
            raise ValueError(f"{who}: background must be finite and >= 0")
        w = per_channel(1.0 if weights is None else weights, "weights")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError(f"{who}: weights must be finite and >= 0")
        sigma = None
        if absorption is not None:
            sigma = np.asarray(absorption, dtype=np.float64)
            if sigma.shape != lo.shape or not np.isfinite(sigma).all() or (sigma < 0).any():
                raise ValueError(f"{who}: absorption must be [{J} bins], finite and >= 0, got shape {sigma.shape}")
        with np.errstate(over="ignore"):
            if m == 1:
                times = (t0 + 0.5 * expo)[:, None]
            else:
                times = t0[:, None] + np.arange(m, dtype=np.float64)[None, :] * (expo / float(m - 1))[:, None]
        if not np.isfinite(times).all():
            raise ValueError(f"{who}: t_start + exposure must be finite")
        t_sample, inverse = np.unique(times.ravel(), return_inverse=True)  # ascending, equal times once
        eom = expo / float(m)
        if not np.isfinite(eom).all() or (eom <= 0).any():
            raise ValueError(f"{who}: exposure / num_exposure_points must be finite and > 0 at every row")
        nu = np.sqrt(lo * hi) * units.keV
        with np.errstate(over="ignore"):
            A = (R * (np.log(hi / lo) / units._PLANCK_ERG_S)[None, :]).T
        if not (np.isfinite(nu).all() and (np.diff(nu) > 0).all() and (nu > 0).all()):
            raise ValueError(f"{who}: the bins of energy_lo / energy_hi do not give distinct, finite nodes sqrt(lo hi)")
        if not np.isfinite(A).all():
            raise ValueError(f"{who}: response * ln(energy_hi / energy_lo) / h must be finite")
        c = np.ascontiguousarray
        self._fold_obs.append(dict(energy_lo=c(lo), energy_hi=c(hi), response=c(R), nu=c(nu), A=c(A), sigma=None if sigma is None else c(sigma),
                                   m=m, t_sample=c(t_sample), sample_idx=c(inverse.reshape(t0.size, m), dtype=np.int32),
                                   exposure_over_m=c(eom), counts=c(N), background=c(bkg), weights=c(w),
                                   const2=float(-2.0 * np.sum(np.where(w > 0, w * _poisson_const(N), 0.0)))))

    @property
    def has_count_spectra(self):
        """Some data are count spectra (add_count_spectrum)."""
        return bool(self._fold_obs)

    def add_centroid(self, nu, t, east, north, err_east, err_north, weights=None):
        """VLBI centroid positions at one frequency nu [Hz]: offsets east / north of a reference position and their errors [rad]
        (units.mas converts) at ascending times t [s].  The group is its own request: the model centroid at (t_i, nu) is
        Model.sky_moments(t, nu, exact=True) placed on the sky by the parameters "pa" (position angle of the jet, east of
        north), "east0" and "north0" (free or fixed; 0 when not given), and adds
        sum_i w_i [((east_i - east) / err_east_i)^2 + ((north_i - north) / err_north_i)^2] to chi^2."""
        nu = float(np.asarray(nu, dtype=np.float64)) if np.ndim(nu) == 0 else None
        if nu is None or not np.isfinite(nu) or nu <= 0:
            raise ValueError("add_centroid: nu must be one finite frequency > 0")
        arrs = [np.asarray(a, dtype=np.float64) for a in (t, east, north, err_east, err_north)]
        t, east, north, err_east, err_north = arrs
        if t.ndim != 1 or t.size == 0:
            raise ValueError("add_centroid: t must be a non-empty 1-D array")
        if any(a.shape != t.shape for a in arrs):
            raise ValueError("add_centroid: t, east, north, err_east, err_north must have the same shape; got "
                             f"{[a.shape for a in arrs]}")
        if not all(np.isfinite(a).all() for a in arrs):
            raise ValueError("add_centroid: t, positions and errors must be finite")
        if (t <= 0).any() or (np.diff(t) < 0).any():
            raise ValueError("add_centroid: times must be > 0 and ascending")
        if (err_east <= 0).any() or (err_north <= 0).any():
            raise ValueError("add_centroid: err_east and err_north must be > 0 at every epoch")
        if weights is None:
            w = np.ones_like(t)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t.shape or not np.isfinite(w).all() or (w < 0).any():
                raise ValueError("add_centroid: weights must have the shape of t and be finite and >= 0")
        self._centroid_obs.append(dict(nu=nu, t=np.ascontiguousarray(t), east=np.ascontiguousarray(east),
                                       north=np.ascontiguousarray(north), err_east=np.ascontiguousarray(err_east),
                                       err_north=np.ascontiguousarray(err_north), weights=np.ascontiguousarray(w)))

    @property
    def has_centroids(self):
        return bool(self._centroid_obs)

    def add_visibilities(self, nu, t, u, v, vis, err, weights=None, n_az=None, kind="complex"):
        """VLBI visibilities at one frequency nu [Hz]: flat arrays with one entry per visibility -- time t [s] (ascending; runs of
        equal t are the epochs, each with its own baselines), baseline u (east) and v (north) [wavelengths], the measured complex
        visibility ``vis`` [erg cm^-2 s^-1 Hz^-1] and ``err``, the standard deviation of its real and of its imaginary part.  The
        group is its own request: the model visibility is Model.sky_visibilities(t, nu, u, v, pa, n_az) times
        exp(-2 pi i (u east0 + v north0)), placed by the parameters "pa", "east0" and "north0" (free or fixed; 0 when not given;
        shared with the centroid groups), and adds sum_k w_k |vis_k - V_mod,k|^2 / err_k^2 to chi^2.  kind="amplitude" is for data
        without usable phases: ``vis`` holds real amplitudes and the term is sum_k w_k (vis_k - |V_mod,k|)^2 / err_k^2.  n_az:
        azimuthal parts per circle of the model (default 1024, Model.sky_visibilities' own; a smaller value makes the fit cheaper
        at the accuracy INTEGRATION.md states).  Weights are used as given."""
        who = "add_visibilities"
        nu = float(np.asarray(nu, dtype=np.float64)) if np.ndim(nu) == 0 else None
        if nu is None or not np.isfinite(nu) or nu <= 0:
            raise ValueError(f"{who}: nu must be one finite frequency > 0")
        if kind not in _lib.VIS_KINDS:
            raise ValueError(f"{who}: kind must be 'complex' or 'amplitude', got {kind!r}")
        if n_az is not None and (int(n_az) != n_az or n_az < 1):
            raise ValueError(f"{who}: n_az must be an integer >= 1 (or None for 1024), got {n_az!r}")
        vis = np.asarray(vis)
        if kind == "amplitude":
            if np.iscomplexobj(vis):
                raise ValueError(f"{who}: kind='amplitude' takes real amplitudes, got complex data")
            vis = vis.astype(np.float64)
        else:
            vis = vis.astype(np.complex128)
        t, u, v, err = (np.asarray(a, dtype=np.float64) for a in (t, u, v, err))
        if t.ndim != 1 or t.size == 0:
            raise ValueError(f"{who}: t must be a non-empty 1-D array")
        if any(a.shape != t.shape for a in (u, v, vis, err)):
            raise ValueError(f"{who}: t, u, v, vis, err must have the same shape; got {[a.shape for a in (t, u, v, vis, err)]}")
        if not all(np.isfinite(a).all() for a in (t, u, v, vis, err)):
            raise ValueError(f"{who}: t, baselines, visibilities and errors must be finite")
        if (t <= 0).any() or (np.diff(t) < 0).any():
            raise ValueError(f"{who}: times must be > 0 and ascending")
        if (err <= 0).any():
            raise ValueError(f"{who}: err must be > 0 at every visibility")
        if weights is None:
            w = np.ones_like(t)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t.shape or not np.isfinite(w).all() or (w < 0).any():
                raise ValueError(f"{who}: weights must have the shape of t and be finite and >= 0")
        starts = np.concatenate(([0], np.nonzero(np.diff(t) > 0)[0] + 1))  # runs of equal t are the epochs
        first = np.ascontiguousarray(np.concatenate((starts, [t.size])), dtype=np.int32)
        c = np.ascontiguousarray
        self._vis_obs.append(dict(nu=nu, t=c(t[starts]), first=first, u=c(u), v=c(v), re=c(vis.real), err=c(err), weights=c(w),
                                  im=c(vis.imag) if kind == "complex" else None, n_az=None if n_az is None else int(n_az),
                                  kind=kind))

    @property
    def has_visibilities(self):
        return bool(self._vis_obs)

    def add_polarization(self, nu, t, q, u=None, err_q=None, err_u=None, weights=None, n_az=None, kind="qu", upper_limit=None):
        """Linear polarization measurements at one frequency nu [Hz] at ascending times t [s].  kind="qu": q = Q/I and u = U/I on
        the sky (IAU, as SkyPolarization.q / .u) with errors err_q, err_u; the group is its own request: the model Stokes values
        are Model.sky_polarization(t, nu, b, pi_max, b_rvs, pi_max_rvs, pa, n_az) with the parameters "pol_b", "pol_pi_max",
        "pol_b_rvs", "pol_pi_max_rvs" (free or fixed; defaults as sky_polarization: b = 0, the reverse shock follows the forward b,
        pi_max from the walker's own p) and "pa" (shared with the centroid and visibility groups), and adds
        sum_i w_i [((q_i - Q/I) / err_q_i)^2 + ((u_i - U/I) / err_u_i)^2] to chi^2.  kind="degree": q holds the polarization degree
        and err_q its error (u, err_u are not used); the term is sum_i w_i ((q_i - hypot(Q, U)/I) / err_q_i)^2 and "pa" drops out.
        n_az: azimuthal parts per circle of the model (default 256, Model.sky_polarization's own).  Weights are used as given.
        upper_limit (kind="degree" only): None, a bool or a boolean mask of the shape of t; on a flagged epoch q is the limit on the
        degree ("Pi < 12 %": q = 0.12) and err_q its noise level, and the term is -2 w ln Phi((q - hypot(Q, U)/I) / err_q)."""
        who = "add_polarization"
        nu = float(np.asarray(nu, dtype=np.float64)) if np.ndim(nu) == 0 else None
        if nu is None or not np.isfinite(nu) or nu <= 0:
            raise ValueError(f"{who}: nu must be one finite frequency > 0")
        if kind not in _lib.POL_KINDS:
            raise ValueError(f"{who}: kind must be 'qu' or 'degree', got {kind!r}")
        if n_az is not None and (int(n_az) != n_az or n_az < 1):
            raise ValueError(f"{who}: n_az must be an integer >= 1 (or None for 256), got {n_az!r}")
        if err_q is None:
            raise ValueError(f"{who}: err_q is required")
        qu = kind == "qu"
        if qu and (u is None or err_u is None):
            raise ValueError(f"{who}: kind='qu' needs u and err_u")
        names = ("t", "q", "err_q") + (("u", "err_u") if qu else ())
        given = dict(t=t, q=q, err_q=err_q, u=u, err_u=err_u)
        arrs = {k: np.asarray(given[k], dtype=np.float64) for k in names}
        t = arrs["t"]
        if t.ndim != 1 or t.size == 0:
            raise ValueError(f"{who}: t must be a non-empty 1-D array")
        if any(a.shape != t.shape for a in arrs.values()):
            raise ValueError(f"{who}: {', '.join(names)} must have the same shape; got {[a.shape for a in arrs.values()]}")
        if not all(np.isfinite(a).all() for a in arrs.values()):
            raise ValueError(f"{who}: t, measurements and errors must be finite")
        if (t <= 0).any() or (np.diff(t) < 0).any():
            raise ValueError(f"{who}: times must be > 0 and ascending")
        if any((arrs[k] <= 0).any() for k in names if k.startswith("err")):
            raise ValueError(f"{who}: errors must be > 0 at every epoch")
        if qu and ((np.abs(arrs["q"]) > 1).any() or (np.abs(arrs["u"]) > 1).any()):
            raise ValueError(f"{who}: |q| and |u| must be <= 1")
        if not qu and ((arrs["q"] < 0).any() or (arrs["q"] > 1).any()):
            raise ValueError(f"{who}: the polarization degree must be in [0, 1]")
        if weights is None:
            w = np.ones_like(t)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != t.shape or not np.isfinite(w).all() or (w < 0).any():
                raise ValueError(f"{who}: weights must have the shape of t and be finite and >= 0")
        lim = self._limit_mask(upper_limit, t, arrs["q"], who)
        if qu and lim.any():
            raise ValueError(f"{who}: upper limits need kind='degree' (limits on q / u are not supported)")
        c = np.ascontiguousarray
        self._pol_obs.append(dict(nu=nu, t=c(t), q=c(arrs["q"]), err_q=c(arrs["err_q"]), u=c(arrs["u"]) if qu else None,
                                  err_u=c(arrs["err_u"]) if qu else None, weights=c(w), n_az=None if n_az is None else int(n_az),
                                  kind=kind, lim=c(lim, dtype=np.int32) if lim.any() else None))

    @property
    def has_polarization(self):
        return bool(self._pol_obs)

    @property
    def has_limits(self):
        """Some row of the data is an upper limit (upper_limit=... of add_flux_density / add_spectrum / add_flux / add_polarization)."""
        return (any(m.any() for m in self._point_lim) or any(bd["lim"] is not None for bd in self._band_obs)
                or any(pd["lim"] is not None for pd in self._pol_obs))

    @property
    def has_noise_groups(self):
        """Some rows belong to a noise group (noise=... of add_flux_density / add_spectrum / add_flux)."""
        return bool(self._noise_labels)

    @property
    def has_outlier_groups(self):
        """Some noise group is robust (outliers=True of add_flux_density / add_spectrum / add_flux)."""
        return any(self._noise_robust.get(label, False) for label in self._noise_labels)

    @property
    def has_templates(self):
        """The fit has additive templates (templates=... of add_flux_density / add_spectrum / add_flux, or add_template)."""
        return bool(self._tmpl_names)

    # fitter.py:407-451
    def _consolidate_data(self):
        if self._all_t is not None:
            return
        if not self._point_t:
            if not (self._band_obs or self._centroid_obs or self._vis_obs or self._pol_obs or self._counts_obs or self._index_obs
                    or self._fold_obs or self._cov_obs):
                raise ValueError("no data: call add_flux_density, add_flux, add_centroid, add_visibilities, add_polarization, "
                                 "add_counts, add_spectral_index, add_count_spectrum or add_correlated first")
            self._all_t = self._all_nu = self._all_log_flux = self._all_log_err = self._all_weights = np.array([])
            self._all_lim = self._all_grp = None
            self._all_tmpl = {}
            return
        t = np.concatenate(self._point_t)
        nu = np.concatenate(self._point_nu)
        f = np.concatenate(self._point_flux)
        e = np.concatenate(self._point_err)
        w = np.concatenate(self._point_weights)
        lim = np.concatenate(self._point_lim)
        order = np.argsort(t)
        t, nu, f, e, w = t[order], nu[order], f[order], e[order], w[order].copy()
        grp = np.concatenate(self._point_grp)[order]  # the noise group ids follow the sort
        self._all_tmpl = {}  # template id -> its values at the consolidated rows (0 where a call did not mention it): they follow the sort
        for c in sorted(set().union(*[set(d) for d in self._point_tmpl])):
            self._all_tmpl[c] = np.concatenate([d[c] if c in d else np.zeros(ti.shape) for d, ti in zip(self._point_tmpl, self._point_t)])[order]
        self._all_grp = np.ascontiguousarray(grp, dtype=np.int32) if (grp >= 0).any() else None
        if lim.any():
            # upper-limit rows: the weights of the DETECTIONS are normalised to sum to their count, as without the limit rows; a limit
            # row keeps its weight as given.  ln_flux / ln_err are not read on a limit row (0 and 1).
            lim = lim[order]
            det = ~lim
            wd = w[det]
            s = wd.sum()
            if s > 0:
                wd *= len(wd) / s
                w[det] = wd
            if np.any(f[det] <= 0) or np.any(e <= 0):
                raise ValueError("the log-flux likelihood requires strictly positive fluxes and errors")
            safe = np.where(lim, 1.0, f)
            self._all_log_flux = np.ascontiguousarray(np.where(lim, 0.0, np.log(safe)))
            self._all_log_err = np.ascontiguousarray(np.where(lim, 1.0, e / safe))
            self._all_lim = dict(kind=np.ascontiguousarray(lim, dtype=np.int32), limit=np.ascontiguousarray(np.where(lim, f, 0.0)),
                                 sigma=np.ascontiguousarray(np.where(lim, e, 1.0)))
        else:
            s = w.sum()
            if s > 0:
                w *= len(w) / s
            if np.any(f <= 0) or np.any(e <= 0):
                raise ValueError("the log-flux likelihood requires strictly positive fluxes and errors")
            self._all_log_flux = np.ascontiguousarray(np.log(f))
            self._all_log_err = np.ascontiguousarray(e / f)
            self._all_lim = None
        self._all_t, self._all_nu = np.ascontiguousarray(t), np.ascontiguousarray(nu)
        self._all_weights = np.ascontiguousarray(w)
        if self.extinction is not None:  # fitter.py:439-449: rest-frame wavelengths, kernel = 0.4 ln10 k(lambda)
            self._ext_z = self.z
            lam_rest_cm = (2.99792458e10 / self._all_nu) / (1.0 + self.z)
            self._ext_kernel = np.ascontiguousarray(0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64))
            self._ext_kernels = {self._ext_z: self._ext_kernel}

    def _k_lambda(self, lam_rest_cm):
        """k(lambda) of the configured law.  The reference hands custom callables (lam_rest_cm, params) (fitter.py:445-449);
        such a two-argument law is called with params=None here, so one that really depends on the sampled parameters
        fails loudly instead of being frozen silently."""
        import inspect
        try:
            n_pos = sum(1 for q in inspect.signature(self.extinction).parameters.values()
                        if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) and q.default is q.empty)
        except (TypeError, ValueError):
            n_pos = 1
        return self.extinction(lam_rest_cm, None) if n_pos >= 2 else self.extinction(lam_rest_cm)

    def _base_params(self, fixed):
        vals = dict(MODEL_PARAM_DEFAULTS)
        vals.update(fixed)
        p = _lib.ModelParams()
        _lib.load().vag_params_default(C.byref(p))
        p.jet_type, p.medium_type = JET_TYPES[self.jet], MEDIUM_TYPES[self.medium]
        p.theta_c, p.E_iso, p.Gamma0, p.k_e, p.k_g = vals["theta_c"], vals["E_iso"], vals["Gamma0"], vals["k_e"], vals["k_g"]
        p.theta_w, p.E_iso_w, p.Gamma0_w, p.duration = vals["theta_w"], vals["E_iso_w"], vals["Gamma0_w"], vals["tau"]
        p.n_ism, p.A_star, p.n0, p.k_m = vals["n_ism"], vals["A_star"], vals["n0"], vals["k_m"]
        if self.jet == "uniform":
            p.theta_c = math.pi / 2
        p.lumi_dist, p.z, p.theta_obs = self.lumi_dist, self.z, vals["theta_v"]
        p.eps_e, p.eps_B, p.p, p.xi_e = vals["eps_e"], vals["eps_B"], vals["p"], vals["xi_e"]
        p.phi_resol, p.theta_resol, p.t_resol = self.resolution
        p.rtol = self.rtol
        p.radiative_fireball = 1 if self.radiative_fireball else 0
        p.flags = (_lib.FLAG_SSC if self.fwd_ssc else 0) | (_lib.FLAG_KN if self.kn else 0)  # fitter.py:466-473
        if self.magnetar and self.jet != "powerlaw_wing":  # fitting/utils.py:47-52: Magnetar(L0, t0, q) on the jets that take one
            p.flags |= _lib.FLAG_MAGNETAR                      # (config.py:99-121: powerlaw_wing has supports_magnetar=False: it is left out)
            p.mag_L0, p.mag_t0, p.mag_q = vals["L0"], vals["t0"], vals["q"]
        if self.rvs_shock:  # fitter.py:476-484: rvs_rad = Radiation(eps_e_r, eps_B_r, p_r, xi_e_r, ssc=rvs_ssc, kn=kn)
            p.flags |= _lib.FLAG_RVS | (_lib.FLAG_RVS_SSC if self.rvs_ssc else 0) | (_lib.FLAG_RVS_KN if self.kn else 0)
            p.rvs_eps_e, p.rvs_eps_B, p.rvs_p, p.rvs_xi_e = vals["eps_e_r"], vals["eps_B_r"], vals["p_r"], vals["xi_e_r"]
        return p

    def build_spec(self, param_defs: Sequence[ParamDef], priors=None, use_priors=False):
        """The transformer of fitting/utils.py:110-135 as a C-ABI slot map (vag_fit_spec).  With ``use_priors`` the spec also
        carries the sampler-space bounds and the priors of fitting/params.py:209-227 (Uniform(lower, upper) unless ``priors``
        names another one), so that the device applies the bounds mask and adds sum ln prior (samplers.py:72-91)."""
        self._consolidate_data()
        self._check_noise_parameters(param_defs)
        self._check_outlier_parameters(param_defs)
        self._check_template_parameters(param_defs)
        fixed = {pd.name: (pd.initial if pd.initial is not None else pd.lower) for pd in param_defs if pd.scale is Scale.fixed}
        free = [pd for pd in param_defs if pd.scale is not Scale.fixed]
        if len(free) > 16:
            raise ValueError("at most 16 free parameters")
        spec = _lib.FitSpec()
        spec.base = self._base_params(fixed)
        # fixed parameters that are Model / Observer fields rather than ModelParams entries (z, lumi_dist, sigma0, the theta_obs /
        # duration aliases ...) go straight into their slot, exactly like a free parameter would
        base_fields = (C.c_double * 40).from_address(C.addressof(spec.base) + _lib.ModelParams.theta_c.offset)
        for name, value in fixed.items():
            if name in MODEL_PARAM_DEFAULTS or name in ("A_V", "N_H") or name in _lib.SKY_SLOTS or name in _lib.POL_SLOTS:
                continue
            if self._noise_id(name) is not None:  # (goes into vag_noise_fit_spec.sys_fixed)
                continue
            if self._outlier_slot(name) is not None:  # (goes into vag_robust_fit_spec.frac_fixed / scale_fixed / shift_fixed)
                continue
            if self._tmpl_id(name) is not None:  # (goes into vag_template_fit_spec.amp_fixed)
                continue
            if name not in _lib.PARAM_SLOTS:
                raise ValueError(f"parameter {name} is not accepted by the accelerated path")
            base_fields[_lib.PARAM_SLOTS[name]] = float(value)
        spec.ndim = len(free)
        for d, pd in enumerate(free):
            if pd.name == "A_V":
                spec.slot[d] = _lib.P_A_V
            elif pd.name == "N_H":
                spec.slot[d] = _lib.P_N_H
            elif pd.name in _lib.SKY_SLOTS:
                spec.slot[d] = _lib.SKY_SLOTS[pd.name]
            elif pd.name in _lib.POL_SLOTS:
                spec.slot[d] = _lib.POL_SLOTS[pd.name]
            elif self._noise_id(pd.name) is not None:
                spec.slot[d] = _lib.P_NOISE_SYS0 + self._noise_id(pd.name)
            elif self._outlier_slot(pd.name) is not None:
                spec.slot[d] = self._outlier_slot(pd.name)
            elif self._tmpl_id(pd.name) is not None:
                spec.slot[d] = _lib.P_TMPL_AMP0 + self._tmpl_id(pd.name)
            elif pd.name not in _lib.PARAM_SLOTS:
                raise ValueError(f"parameter {pd.name} is not accepted by the accelerated path")
            else:
                spec.slot[d] = _lib.PARAM_SLOTS[pd.name]
            spec.is_log[d] = 1 if pd.scale is Scale.log else 0
        spec.a_v_fixed = float(fixed.get("A_V", 0.0))
        self._check_sky_parameters(param_defs)
        # (a fit with visibility or polarization groups only still carries the fixed placement in a vag_sky_fit_spec without groups)
        spec._sky = self._sky_spec(fixed) if self._centroid_obs or self._vis_obs or self._pol_obs else None
        spec._vis = self._vis_spec() if self._vis_obs else None
        spec._pol = self._pol_spec(fixed) if self._pol_obs else None
        spec._lim = self._lim_spec() if self.has_limits else None
        spec._noise = self._noise_spec(fixed) if self.has_noise_groups else None
        spec._robust = self._robust_spec(fixed) if self.has_outlier_groups else None
        spec._counts = self._counts_spec() if self._counts_obs else None
        spec._tmpl = self._tmpl_spec(fixed) if self.has_templates else None
        if self.extinction is not None and any(pd.name == "z" for pd in free):
            raise ValueError("a free 'z' cannot be combined with Fitter(extinction=...): the law's rest-frame wavelengths are fixed per fit")
        z_eff = float(fixed.get("z", self.z))
        spec._index = self._index_spec(z_eff) if self._index_obs else None
        self._check_n_h_parameter(param_defs)
        spec._fold = self._fold_spec(fixed) if self._fold_obs else None
        spec._cov = self._cov_spec(z_eff) if self._cov_obs else None
        if self.extinction is not None and self._all_t.size and z_eff != self._ext_z:
            # a fixed 'z' ParamDef overrides Fitter.z in the model: the rest-frame wavelengths of the law must follow it.  One
            # kernel per z, all kept for the Fitter's lifetime: earlier specs (a device_evaluator's closure) still point at theirs
            ext = self._ext_kernels.get(z_eff)
            if ext is None:
                lam_rest_cm = (2.99792458e10 / self._all_nu) / (1.0 + z_eff)
                ext = self._ext_kernels[z_eff] = np.ascontiguousarray(
                    0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64))
            self._ext_z, self._ext_kernel = z_eff, ext
        spec.ext_kernel = self._ext_kernel.ctypes.data_as(_dp) if self._ext_kernel is not None else None
        self._band_structs = (_lib.BandObs * max(len(self._band_obs), 1))()
        for g, bd in enumerate(self._band_obs):
            b = self._band_structs[g]
            b.nu_min, b.nu_max, b.num_points, b.n = bd["nu_min"], bd["nu_max"], bd["num_points"], bd["t"].size
            b.t, b.ln_flux = bd["t"].ctypes.data_as(_dp), bd["ln_flux"].ctypes.data_as(_dp)
            b.ln_err, b.weight = bd["ln_err"].ctypes.data_as(_dp), bd["weights"].ctypes.data_as(_dp)
        spec.n_bands = len(self._band_obs)
        spec.bands = self._band_structs
        spec.n_data = self._all_t.size
        spec.t = self._all_t.ctypes.data_as(_dp)
        spec.nu = self._all_nu.ctypes.data_as(_dp)
        spec.ln_flux = self._all_log_flux.ctypes.data_as(_dp)
        spec.ln_err = self._all_log_err.ctypes.data_as(_dp)
        spec.weight = self._all_weights.ctypes.data_as(_dp)
        # the struct holds raw pointers: what they point at lives as long as the spec (a device_evaluator closure keeps its spec
        # while the Fitter may consolidate new data or another z)
        spec._keep_alive = (self._ext_kernel, self._band_structs, list(self._band_obs), self._all_t, self._all_nu,
                            self._all_log_flux, self._all_log_err, self._all_weights)
        # sampler-space bounds: log10 of the ParamDef bounds for LOG-scale parameters (fitting/params.py:196-201)
        lower = np.array([np.log10(pd.lower) if pd.scale is Scale.log else pd.lower for pd in free], dtype=np.float64)
        upper = np.array([np.log10(pd.upper) if pd.scale is Scale.log else pd.upper for pd in free], dtype=np.float64)
        self._host_priors, self._prior_specs = [], []
        spec.use_priors = 1 if use_priors else 0
        for d, pd in enumerate(free):
            spec.lower[d], spec.upper[d] = lower[d], upper[d]
            kind, a, b = _device_prior((priors or {}).get(pd.name))
            if kind == _lib.PRIOR_NONE:
                self._host_priors.append((d, priors[pd.name]))
            self._prior_specs.append((kind, a, b, (priors or {}).get(pd.name)))
            spec.prior_kind[d], spec.prior_a[d], spec.prior_b[d] = kind, a, b
        return spec, lower, upper

    def _sky_spec(self, fixed):
        """vag_sky_fit_spec of the centroid groups; it keeps the arrays it points at alive."""
        sky = _lib.SkyFitSpec()
        groups = (_lib.CentroidObs * max(len(self._centroid_obs), 1))()
        for g, cd in enumerate(self._centroid_obs):
            o = groups[g]
            o.nu, o.n = cd["nu"], cd["t"].size
            for name in ("t", "east", "north", "err_east", "err_north"):
                setattr(o, name, cd[name].ctypes.data_as(_dp))
            o.weight = cd["weights"].ctypes.data_as(_dp)
        sky.n_groups, sky.groups = len(self._centroid_obs), groups
        sky.pa_fixed, sky.east0_fixed, sky.north0_fixed = (float(fixed.get(k, 0.0)) for k in ("pa", "east0", "north0"))
        sky._keep_alive = (groups, list(self._centroid_obs))
        return sky

    def _counts_spec(self):
        """vag_counts_fit_spec of the counts groups; it keeps the arrays it points at alive."""
        cs = _lib.CountsFitSpec()
        groups = (_lib.CountsObs * len(self._counts_obs))()
        for g, cd in enumerate(self._counts_obs):
            o = groups[g]
            o.nu_min, o.nu_max, o.num_points = cd["nu_min"], cd["nu_max"], cd["num_points"]
            o.n, o.m, o.n_samples = cd["counts"].size, cd["m"], cd["t_sample"].size
            o.t_sample = cd["t_sample"].ctypes.data_as(_dp)
            o.sample_idx = cd["sample_idx"].ctypes.data_as(C.POINTER(C.c_int32))
            for name in ("counts", "background", "scale"):
                setattr(o, name, cd[name].ctypes.data_as(_dp))
            o.weight = cd["weights"].ctypes.data_as(_dp)
        cs.n_groups, cs.groups = len(self._counts_obs), groups
        cs._keep_alive = (groups, list(self._counts_obs))
        return cs

    def _check_n_h_parameter(self, param_defs):
        """N_H is read by count-spectrum groups with absorption only; a fixed one is >= 0, a free one has lower >= 0."""
        for pd in param_defs:
            if pd.name != "N_H":
                continue
            if not any(gd["sigma"] is not None for gd in self._fold_obs):
                raise ValueError("the parameter 'N_H' needs count spectra with a cross-section (Fitter.add_count_spectrum(..., "
                                 "absorption=...))")
            if pd.scale is Scale.fixed:
                value = pd.initial if pd.initial is not None else pd.lower
                if not np.isfinite(value) or value < 0:
                    raise ValueError(f"a fixed N_H must be finite and >= 0, got {value!r}")
            elif not pd.lower >= 0:
                raise ValueError(f"N_H: a free column needs lower >= 0, got lower={pd.lower!r}")

    def _fold_spec(self, fixed):
        """vag_fold_fit_spec of the count-spectrum groups and the fixed N_H; it keeps the arrays it points at alive."""
        fs = _lib.FoldFitSpec()
        groups = (_lib.FoldObs * len(self._fold_obs))()
        for g, gd in enumerate(self._fold_obs):
            o = groups[g]
            o.J, o.C, o.n, o.m, o.n_samples = gd["nu"].size, gd["A"].shape[1], gd["exposure_over_m"].size, gd["m"], gd["t_sample"].size
            for name in ("nu", "A", "t_sample", "exposure_over_m", "counts", "background"):
                setattr(o, name, gd[name].ctypes.data_as(_dp))
            o.sigma = gd["sigma"].ctypes.data_as(_dp) if gd["sigma"] is not None else None
            o.sample_idx = gd["sample_idx"].ctypes.data_as(C.POINTER(C.c_int32))
            o.weight = gd["weights"].ctypes.data_as(_dp)
        fs.n_groups, fs.groups = len(self._fold_obs), groups
        fs.n_h_fixed = float(fixed.get("N_H", self.n_h))
        fs._keep_alive = (groups, list(self._fold_obs))
        return fs

    def _cov_ext(self, gd, z):
        """The extinction kernel 0.4 ln10 k(lambda_rest) at the rows of a correlated group at redshift z, formed as for the point
        rows; None without an extinction law."""
        if self.extinction is None:
            return None
        lam_rest_cm = (2.99792458e10 / gd["nu"]) / (1.0 + z)
        return np.ascontiguousarray(0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64))

    def _cov_spec(self, z):
        """vag_cov_fit_spec of the correlated groups (the law's kernel at redshift z); it keeps the arrays it points at alive."""
        cs = _lib.CovFitSpec()
        groups = (_lib.CovObs * len(self._cov_obs))()
        exts = []
        for g, gd in enumerate(self._cov_obs):
            o = groups[g]
            o.n, o.weight = gd["t"].size, gd["weight"]
            for name in ("t", "nu", "ln_flux", "whitener"):
                setattr(o, name, gd[name].ctypes.data_as(_dp))
            exts.append(self._cov_ext(gd, z))
            o.ext = exts[-1].ctypes.data_as(_dp) if exts[-1] is not None else None
        cs.n_groups, cs.groups = len(self._cov_obs), groups
        cs._keep_alive = (groups, list(self._cov_obs), exts)
        return cs

    def _index_ext_slope(self, gd, z):
        """ext_slope of a spectral-index group at redshift z: sum_{k >= 1} c_k (kappa_k - kappa_0), kappa = 0.4 ln10 k(lambda_rest),
        the kernel of the point rows; 0 without an extinction law."""
        if self.extinction is None:
            return 0.0
        lam_rest_cm = (2.99792458e10 / gd["nu"]) / (1.0 + z)
        kappa = 0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64)
        s = 0.0
        for k in range(1, kappa.size):
            s = s + gd["coef"][k] * (kappa[k] - kappa[0])
        return float(s)

    def _index_spec(self, z):
        """vag_index_fit_spec of the spectral-index groups (the law's reddening at redshift z); it keeps the arrays it points at
        alive."""
        ispec = _lib.IndexFitSpec()
        groups = (_lib.IndexObs * len(self._index_obs))()
        for g, gd in enumerate(self._index_obs):
            o = groups[g]
            o.n, o.k, o.ext_slope = gd["t"].size, gd["nu"].size, self._index_ext_slope(gd, z)
            for name in ("nu", "coef", "t", "value", "err"):
                setattr(o, name, gd[name].ctypes.data_as(_dp))
            o.weight = gd["weights"].ctypes.data_as(_dp)
        ispec.n_groups, ispec.groups = len(self._index_obs), groups
        ispec._keep_alive = (groups, list(self._index_obs))
        return ispec

    def _vis_spec(self):
        """vag_vis_fit_spec of the visibility groups; it keeps the arrays it points at alive."""
        vis = _lib.VisFitSpec()
        groups = (_lib.VisibilityObs * len(self._vis_obs))()
        for g, vd in enumerate(self._vis_obs):
            o = groups[g]
            o.nu, o.n_epochs, o.n_vis = vd["nu"], vd["t"].size, vd["u"].size
            o.n_az, o.kind = vd["n_az"] or 0, _lib.VIS_KINDS[vd["kind"]]
            o.first = vd["first"].ctypes.data_as(C.POINTER(C.c_int32))
            for name in ("t", "u", "v", "re", "err"):
                setattr(o, name, vd[name].ctypes.data_as(_dp))
            o.im = vd["im"].ctypes.data_as(_dp) if vd["im"] is not None else None
            o.weight = vd["weights"].ctypes.data_as(_dp)
        vis.n_groups, vis.groups = len(self._vis_obs), groups
        vis._keep_alive = (groups, list(self._vis_obs))
        return vis

    def _check_sky_parameters(self, param_defs):
        """The parameters that are read by sky data only need such data."""
        names = [pd.name for pd in param_defs]
        placed = self._centroid_obs or self._vis_obs
        self._check_pol_parameters(names)
        if "pa" in names and not placed and not self._pol_obs:
            raise ValueError("the parameters 'pa', 'east0' and 'north0' need centroid data (Fitter.add_centroid) or visibility "
                             "data (Fitter.add_visibilities); 'pa' is also read by polarization data (Fitter.add_polarization)")
        if any(n in ("east0", "north0") for n in names) and not placed:
            raise ValueError("the parameters 'east0' and 'north0' need centroid data (Fitter.add_centroid) or visibility data "
                             "(Fitter.add_visibilities)")

    def _check_pol_parameters(self, names):
        if any(n in _lib.POL_SLOTS for n in names) and not self._pol_obs:
            raise ValueError("the parameters 'pol_b', 'pol_pi_max', 'pol_b_rvs' and 'pol_pi_max_rvs' need polarization data "
                             "(Fitter.add_polarization)")

    def _pol_spec(self, fixed):
        """vag_pol_fit_spec of the polarization groups and the fixed field parameters; it keeps the arrays it points at alive."""
        pol = _lib.PolFitSpec()
        groups = (_lib.PolarizationObs * len(self._pol_obs))()
        for g, pd in enumerate(self._pol_obs):
            o = groups[g]
            o.nu, o.n, o.n_az, o.kind = pd["nu"], pd["t"].size, pd["n_az"] or 0, _lib.POL_KINDS[pd["kind"]]
            for name in ("t", "q", "u", "err_q", "err_u"):
                setattr(o, name, pd[name].ctypes.data_as(_dp) if pd[name] is not None else None)
            o.weight = pd["weights"].ctypes.data_as(_dp)
        pol.n_groups, pol.groups = len(self._pol_obs), groups
        # the defaults of Model.sky_polarization: b = 0, the reverse shock follows the forward b (< 0), pi_max from p (< 0)
        pol.b_fixed[0], pol.b_fixed[1] = float(fixed.get("pol_b", 0.0)), float(fixed.get("pol_b_rvs", -1.0))
        pol.pi_max_fixed[0], pol.pi_max_fixed[1] = float(fixed.get("pol_pi_max", -1.0)), float(fixed.get("pol_pi_max_rvs", -1.0))
        for name in _lib.POL_SLOTS:
            if name in fixed and (not np.isfinite(fixed[name]) or fixed[name] < 0 or (name.startswith("pol_pi_max") and fixed[name] > 1)):
                raise ValueError(f"a fixed {name} must be finite and >= 0" + (" and <= 1" if name.startswith("pol_pi_max") else ""))
        pol._keep_alive = (groups, list(self._pol_obs))
        return pol

    def _noise_id(self, name):
        """The group id of the parameter name ``sys_<label>`` of a declared noise group, else None."""
        if not name.startswith(_lib.NOISE_PREFIX) or name[len(_lib.NOISE_PREFIX):] not in self._noise_labels:
            return None
        return self._noise_labels.index(name[len(_lib.NOISE_PREFIX):])

    def _check_noise_parameters(self, param_defs):
        """``sys_<label>`` needs the noise group <label>; a fixed one is >= 0, a free one has lower >= 0 (> 0 on log scale)."""
        for pd in param_defs:
            if not pd.name.startswith(_lib.NOISE_PREFIX):
                continue
            if self._noise_id(pd.name) is None:
                raise ValueError(f"the parameter {pd.name!r} needs data added with noise={pd.name[len(_lib.NOISE_PREFIX):]!r} "
                                 f"(declared noise groups: {self._noise_labels})")
            if pd.scale is Scale.fixed:
                value = pd.initial if pd.initial is not None else pd.lower
                if not np.isfinite(value) or value < 0:
                    raise ValueError(f"a fixed {pd.name} must be finite and >= 0, got {value!r}")
            elif not pd.lower >= 0 or (pd.scale is Scale.log and not pd.lower > 0):
                raise ValueError(f"{pd.name}: a free systematic needs lower >= 0 (> 0 on log scale), got lower={pd.lower!r}")

    def _noise_spec(self, fixed):
        """vag_noise_fit_spec of the noise groups: the group ids of the consolidated point rows and of the band groups, the fixed
        systematics and the calibration fractions; it keeps the arrays it points at alive.  A group with a calibration fraction
        must lie in one pass of the likelihood call -- point rows only, or exactly one band group."""
        ip = C.POINTER(C.c_int32)
        nz = _lib.NoiseFitSpec()
        nz.n_groups, nz.n_bands = len(self._noise_labels), len(self._band_obs)
        band_ids = np.ascontiguousarray([bd["noise"] for bd in self._band_obs], dtype=np.int32)
        for g, label in enumerate(self._noise_labels):
            nz.sys_fixed[g] = float(fixed.get(_lib.NOISE_PREFIX + label, 0.0))
            nz.calib[g] = float(self._noise_calib.get(label, 0.0))
            passes = int(self._all_grp is not None and bool((self._all_grp == g).any())) + int((band_ids == g).sum())
            if nz.calib[g] > 0 and passes > 1:
                raise ValueError(f"noise group {label!r} has calibration={nz.calib[g]!r} and rows in {passes} passes of the "
                                 "likelihood call: a group with a calibration fraction must hold point rows only (add_flux_density / "
                                 "add_spectrum) or exactly one add_flux call")
        nz.point_group = self._all_grp.ctypes.data_as(ip) if self._all_grp is not None else None
        nz.band_group = band_ids.ctypes.data_as(ip) if band_ids.size else None
        nz._keep_alive = (self._all_grp, band_ids)
        return nz

    def _outlier_slot(self, name):
        """The slot of the parameter name ``out_frac_<label>`` / ``out_scale_<label>`` / ``out_shift_<label>`` of a robust noise
        group, else None."""
        for prefix, slot0 in _lib.ROBUST_PREFIXES.items():
            label = name[len(prefix):]
            if name.startswith(prefix) and label in self._noise_labels and self._noise_robust.get(label, False):
                return slot0 + self._noise_labels.index(label)
        return None

    def _check_outlier_parameters(self, param_defs):
        """``out_frac_<label>``, ``out_scale_<label>`` and ``out_shift_<label>`` need the robust noise group <label>.  out_frac: free on
        linear scale with lower >= 0 and upper < 1, on log scale with lower > 0 (and upper < 1), or fixed in [0, 1); out_scale: free
        on linear scale with lower >= 0, on log scale, or fixed >= 0; out_shift: free on linear scale only, or fixed and finite."""
        for pd in param_defs:
            prefix = next((q for q in _lib.ROBUST_PREFIXES if pd.name.startswith(q)), None)
            if prefix is None:
                continue
            if self._outlier_slot(pd.name) is None:
                robust = [label for label in self._noise_labels if self._noise_robust.get(label, False)]
                raise ValueError(f"the parameter {pd.name!r} needs data added with noise={pd.name[len(prefix):]!r}, outliers=True "
                                 f"(robust noise groups: {robust})")
            if pd.scale is Scale.fixed:
                value = pd.initial if pd.initial is not None else pd.lower
                if prefix == "out_frac_" and (not np.isfinite(value) or value < 0 or not value < 1):
                    raise ValueError(f"a fixed {pd.name} must be finite and in [0, 1), got {value!r}")
                if prefix == "out_scale_" and (not np.isfinite(value) or value < 0):
                    raise ValueError(f"a fixed {pd.name} must be finite and >= 0, got {value!r}")
                if prefix == "out_shift_" and not np.isfinite(value):
                    raise ValueError(f"a fixed {pd.name} must be finite, got {value!r}")
            elif prefix == "out_frac_":
                if not pd.lower >= 0 or (pd.scale is Scale.log and not pd.lower > 0) or not pd.upper < 1:
                    raise ValueError(f"{pd.name}: a free outlier fraction needs lower >= 0 (> 0 on log scale) and upper < 1, got "
                                     f"[{pd.lower!r}, {pd.upper!r}]")
            elif prefix == "out_scale_":
                if not pd.lower >= 0 or (pd.scale is Scale.log and not pd.lower > 0):
                    raise ValueError(f"{pd.name}: a free outlier scatter needs lower >= 0 (> 0 on log scale), got lower={pd.lower!r}")
            elif pd.scale is Scale.log:
                raise ValueError(f"{pd.name}: the outlier offset is free on linear scale only (it may be negative)")

    def _robust_spec(self, fixed):
        """vag_robust_fit_spec of the robust noise groups: the mask and the fixed outlier fractions, scatters and offsets (0 when
        not given)."""
        rb = _lib.RobustFitSpec()
        rb.n_groups = len(self._noise_labels)
        mask = 0
        for g, label in enumerate(self._noise_labels):
            if not self._noise_robust.get(label, False):
                continue
            if self._noise_calib.get(label, 0.0) > 0:
                raise ValueError(f"noise group {label!r} has outliers=True and calibration={self._noise_calib[label]!r}: the marginalised "
                                 "scale does not commute with the mixture")
            mask |= 1 << g
            rb.frac_fixed[g] = float(fixed.get("out_frac_" + label, 0.0))
            rb.scale_fixed[g] = float(fixed.get("out_scale_" + label, 0.0))
            rb.shift_fixed[g] = float(fixed.get("out_shift_" + label, 0.0))
        rb.mask = mask
        return rb

    def _tmpl_id(self, name):
        """The id of the parameter name ``amp_<name>`` of a declared template, else None."""
        if not name.startswith(_lib.TMPL_PREFIX) or name[len(_lib.TMPL_PREFIX):] not in self._tmpl_names:
            return None
        return self._tmpl_names.index(name[len(_lib.TMPL_PREFIX):])

    def _check_template_parameters(self, param_defs):
        """``amp_<name>`` needs the template <name>; a fixed one is >= 0, a free one has lower >= 0 (> 0 on log scale)."""
        for pd in param_defs:
            if not pd.name.startswith(_lib.TMPL_PREFIX):
                continue
            if self._tmpl_id(pd.name) is None:
                raise ValueError(f"the parameter {pd.name!r} needs the template {pd.name[len(_lib.TMPL_PREFIX):]!r} (templates=... of "
                                 f"add_flux_density / add_spectrum / add_flux, or add_template; declared templates: {self._tmpl_names})")
            if pd.scale is Scale.fixed:
                value = pd.initial if pd.initial is not None else pd.lower
                if not np.isfinite(value) or value < 0:
                    raise ValueError(f"a fixed {pd.name} must be finite and >= 0, got {value!r}")
            elif not pd.lower >= 0 or (pd.scale is Scale.log and not pd.lower > 0):
                raise ValueError(f"{pd.name}: a free amplitude needs lower >= 0 (> 0 on log scale), got lower={pd.lower!r}")

    def _tmpl_spec(self, fixed):
        """vag_template_fit_spec of the templates: their values at the consolidated point rows and at the rows of the band groups
        (0 where a template does not touch a row), the fixed amplitudes and the flags; it keeps the arrays it points at alive."""
        tp = _lib.TemplateFitSpec()
        nt = len(self._tmpl_names)
        tp.n_templates = nt
        for c, name in enumerate(self._tmpl_names):
            tp.amp_fixed[c] = float(fixed.get(_lib.TMPL_PREFIX + name, 0.0))
            tp.extinguished[c] = 1 if self._tmpl_ext[c] else 0
        keep = []
        if self._all_tmpl:
            point = np.zeros((nt, self._all_t.size))
            for c, v in self._all_tmpl.items():
                point[c] = v
            tp.point = point.ctypes.data_as(_dp)
            keep.append(point)
        if any(bd.get("tmpl") for bd in self._band_obs):
            bands = (_dp * len(self._band_obs))()
            for g, bd in enumerate(self._band_obs):
                if not bd.get("tmpl"):
                    continue  # (a null pointer: no template touches the group)
                block = np.zeros((nt, bd["t"].size))
                for c, v in bd["tmpl"].items():
                    block[c] = v
                bands[g] = block.ctypes.data_as(_dp)
                keep.append(block)
            tp.n_bands, tp.bands = len(self._band_obs), bands
            keep.append(bands)
        tp._keep_alive = keep
        return tp

    def template_amplitudes(self, sample, param_defs):
        """{name: amplitude} of every template at a point of sampler space, in linear units (10^value for a log-scale parameter,
        the fixed value, 0 when the parameter is not given): what multiplies the template's values in the model."""
        spec, _, _ = self.build_spec(param_defs)
        sample = np.asarray(sample, dtype=np.float64).reshape(-1)
        if sample.size != spec.ndim:
            raise ValueError(f"expected {spec.ndim} free parameters, got {sample.size}")
        out = {name: (float(spec._tmpl.amp_fixed[c]) if spec._tmpl is not None else 0.0) for c, name in enumerate(self._tmpl_names)}
        for d in range(spec.ndim):
            c = spec.slot[d] - _lib.P_TMPL_AMP0
            if 0 <= c < len(self._tmpl_names):
                out[self._tmpl_names[c]] = float(10.0 ** sample[d] if spec.is_log[d] else sample[d])
        return out

    def _lim_spec(self):
        """vag_limit_fit_spec of the upper-limit rows (parallel to the consolidated point rows, the band groups and the polarization
        groups); it keeps the arrays it points at alive."""
        ip = C.POINTER(C.c_int32)
        lim = _lib.LimitFitSpec()
        keep = []

        def fill(rows, d):
            rows.kind, rows.limit, rows.sigma = d["kind"].ctypes.data_as(ip), d["limit"].ctypes.data_as(_dp), d["sigma"].ctypes.data_as(_dp)
            keep.append(d)
        if self._all_lim is not None:
            fill(lim.point, self._all_lim)
        if any(bd["lim"] is not None for bd in self._band_obs):
            bands = (_lib.LimitRows * len(self._band_obs))()
            for g, bd in enumerate(self._band_obs):
                if bd["lim"] is not None:
                    fill(bands[g], dict(kind=bd["lim"], limit=bd["limit"], sigma=bd["sigma"]))
            lim.n_bands, lim.bands = len(self._band_obs), bands
            keep.append(bands)
        if any(pd["lim"] is not None for pd in self._pol_obs):
            kinds = (ip * len(self._pol_obs))()
            for g, pd in enumerate(self._pol_obs):
                if pd["lim"] is not None:
                    kinds[g] = pd["lim"].ctypes.data_as(ip)
                    keep.append(pd["lim"])
            lim.n_pol_groups, lim.pol_kind = len(self._pol_obs), kinds
            keep.append(kinds)
        lim._keep_alive = keep
        return lim

    def polarization(self, best_params, param_defs, resolution=None):
        """The model polarization at the epochs of every polarization group at a point of sampler space: a list of
        SkyPolarization, one per group, each one Model.sky_polarization request at the group's epochs, frequency and n_az with
        the sample's pa and field parameters."""
        spec, _, _ = self.build_spec(param_defs)
        sample = np.asarray(best_params, dtype=np.float64).reshape(-1)
        vals = dict(pa=spec._sky.pa_fixed if spec._sky is not None else 0.0, pol_b=0.0, pol_pi_max=None, pol_b_rvs=None,
                    pol_pi_max_rvs=None)
        if spec._pol is not None:
            vals["pol_b"] = spec._pol.b_fixed[0]
            vals["pol_b_rvs"] = spec._pol.b_fixed[1] if spec._pol.b_fixed[1] >= 0 else None
            vals["pol_pi_max"] = spec._pol.pi_max_fixed[0] if spec._pol.pi_max_fixed[0] >= 0 else None
            vals["pol_pi_max_rvs"] = spec._pol.pi_max_fixed[1] if spec._pol.pi_max_fixed[1] >= 0 else None
        by_slot = {slot: name for name, slot in {**_lib.SKY_SLOTS, **_lib.POL_SLOTS}.items()}
        for d in range(spec.ndim):
            if by_slot.get(spec.slot[d]) in vals:
                vals[by_slot[spec.slot[d]]] = 10.0 ** sample[d] if spec.is_log[d] else sample[d]
        model = self.model(best_params, param_defs, resolution)
        return [model.sky_polarization(pd["t"], pd["nu"], b=vals["pol_b"], pi_max=vals["pol_pi_max"], b_rvs=vals["pol_b_rvs"],
                                       pi_max_rvs=vals["pol_pi_max_rvs"], pa=vals["pa"], n_az=pd["n_az"]) for pd in self._pol_obs]

    def counts(self, best_params, param_defs, resolution=None):
        """The expected counts mu of every counts group at a point of sampler space: a list of float64 arrays, one per group, in
        the order the rows were added.  Each group is one vag_flux_batch request on the group's merged sample times;
        mu_i = background_i + scale_i * sum_k F[sample_idx[i, k]], summed in k order.  The likelihood forms mu the same way on the
        same request, but with its flux workgroups at a pinned size (so that a walker's term does not depend on the batch):
        the two agree to rounding (1e-15 relative), not to the bits."""
        p, _ = self._params_at(best_params, param_defs, resolution)
        h, lock = get_context(self.device)
        out = []
        for cd in self._counts_obs:
            ts = cd["t_sample"]
            flux = np.empty(ts.size)
            with lock:  # (vag_flux_batch: the total of the enabled components as the likelihood's own band request forms it)
                _lib.check(_lib.load().vag_flux_batch(h, C.byref(p), 1, ts.ctypes.data_as(_dp), ts.size, cd["nu_min"], cd["nu_max"],
                                                      cd["num_points"], flux.ctypes.data_as(_dp)))
            total = np.zeros(cd["counts"].size)
            for k in range(cd["m"]):
                total = total + flux[cd["sample_idx"][:, k]]
            out.append(cd["background"] + cd["scale"] * total)
        return out

    def spectral_indices(self, best_params, param_defs, resolution=None):
        """The model index of every row of every spectral-index group at a point of sampler space, in the group's own convention
        and with the A_V term: a list of float64 arrays, one per group, rows in ascending t.  Each group is one
        vag_flux_density_batch request at its n K points (t_i, nu_k), i outer, and index_slope on the result -- the likelihood's
        own request and arithmetic (its flux may differ from this call's in the last bits)."""
        p, a_v = self._params_at(best_params, param_defs, resolution)
        h, lock = get_context(self.device)
        out = []
        for gd in self._index_obs:
            n, K = gd["t"].size, gd["nu"].size
            ts, nus = np.ascontiguousarray(np.repeat(gd["t"], K)), np.ascontiguousarray(np.tile(gd["nu"], n))
            flux = np.empty(n * K)
            with lock:
                _lib.check(_lib.load().vag_flux_density_batch(h, C.byref(p), 1, ts.ctypes.data_as(_dp), nus.ctypes.data_as(_dp), n * K,
                                                              flux.ctypes.data_as(_dp)))
            slope = index_slope(flux.reshape(n, K), gd["coef"]) - a_v * self._index_ext_slope(gd, float(p.z))
            out.append(index_from_slope(slope, gd["convention"]))
        return out

    def correlated(self, best_params, param_defs, resolution=None):
        """Every correlated group at a point of sampler space: a list of dict(model=f, residual=r, whitened=y, chi2=w sum y^2), one per
        group, rows in ascending t; f is the model flux density with extinction applied, r = ln f_nu - ln max(f, 1e-300), y = W r.
        Each group is one vag_flux_density_batch request at its rows and whitened_chi2's arithmetic on the result -- the
        likelihood's own request and arithmetic (its flux may differ from this call's in the last bits: 1e-15 relative, as
        Fitter.counts documents for an unpinned request)."""
        p, a_v = self._params_at(best_params, param_defs, resolution)
        h, lock = get_context(self.device)
        out = []
        for gd in self._cov_obs:
            n = gd["t"].size
            flux = np.empty(n)
            with lock:
                _lib.check(_lib.load().vag_flux_density_batch(h, C.byref(p), 1, gd["t"].ctypes.data_as(_dp), gd["nu"].ctypes.data_as(_dp), n,
                                                              flux.ctypes.data_as(_dp)))
            ext = self._cov_ext(gd, float(p.z))
            f = flux * np.exp(-a_v * ext) if ext is not None and a_v != 0.0 else flux
            with np.errstate(all="ignore"):
                r = gd["ln_flux"] - np.log(np.where(f > 1e-300, f, np.where(np.isnan(f), f, 1e-300)))
            W = gd["whitener"]
            y = np.zeros(n)
            for j in range(n):  # y_i = sum_{j <= i} W_ij r_j, ascending j (W is lower triangular)
                y = y + W[:, j] * r[j]
            out.append(dict(model=f, residual=r, whitened=y, chi2=gd["weight"] * float(whitened_chi2(r, W))))
        return out

    def outlier_probabilities(self, best_params, param_defs, resolution=None):
        """The posterior probability, row by row, that a point of a robust noise group is an outlier, at a point of sampler space: a
        list of dict(label, t, nu, band, residual, p_out), one per robust group in the order of the noise groups.  The rows are the
        group's point rows in ascending t (``nu`` their frequency, ``band`` -1) followed by the rows of its band groups (``nu`` NaN,
        ``band`` the index of the add_flux call).  residual = ln F_obs - ln max(f, 1e-300) with f the model value as the likelihood
        forms it (templates, then extinction); p_out = exp(o - l) of outlier_terms at the sample's sys, out_frac, out_scale and
        out_shift of the group.  Upper-limit rows carry NaN in both.  The model values come from the device -- one
        vag_flux_density_batch request at the point rows, one vag_flux_batch request per band group, as Fitter.correlated and
        Fitter.counts get theirs -- and the probabilities from outlier_terms on the host."""
        spec, _, _ = self.build_spec(param_defs)
        if spec._robust is None:
            return []
        p, a_v = self._params_at(best_params, param_defs, resolution)
        sample = np.asarray(best_params, dtype=np.float64).reshape(-1)
        labels = self._noise_labels
        par = {g: dict(s=float(spec._noise.sys_fixed[g]), frac=float(spec._robust.frac_fixed[g]), scale=float(spec._robust.scale_fixed[g]),
                       shift=float(spec._robust.shift_fixed[g])) for g in range(len(labels)) if (spec._robust.mask >> g) & 1}
        families = (("s", _lib.P_NOISE_SYS0), ("frac", _lib.P_ROBUST_FRAC0), ("scale", _lib.P_ROBUST_SCALE0), ("shift", _lib.P_ROBUST_SHIFT0))
        amp = np.array([float(spec._tmpl.amp_fixed[c]) if spec._tmpl is not None else 0.0 for c in range(len(self._tmpl_names))])
        for d in range(spec.ndim):
            val = 10.0 ** sample[d] if spec.is_log[d] else sample[d]
            for key, slot0 in families:
                if spec.slot[d] - slot0 in par and 0 <= spec.slot[d] - slot0 < _lib.NOISE_MAX_GROUPS:
                    par[spec.slot[d] - slot0][key] = float(val)
            if 0 <= spec.slot[d] - _lib.P_TMPL_AMP0 < amp.size:
                amp[spec.slot[d] - _lib.P_TMPL_AMP0] = val
        h, lock = get_context(self.device)
        lib = _lib.load()

        def with_templates(F, tmpl, ext):
            """(F + x) exp(-A_V k) + e at the rows of one pass; tmpl: {template id: values}."""
            e = x = 0.0
            if tmpl:
                T = np.zeros((amp.size, F.size))
                for c, v in tmpl.items():
                    T[c] = v
                e, x = template_terms(T, amp, self._tmpl_ext)
            f = F + x
            if ext is not None and a_v != 0.0:
                f = f * np.exp(-a_v * ext)
            return f + e

        def rows_of(f, ln_flux, ln_err, w, lim, g):
            """(residual, p_out) of the rows of one pass that belong to group g; limit rows NaN."""
            with np.errstate(all="ignore"):
                r = ln_flux - np.log(np.where(f > 1e-300, f, np.where(np.isnan(f), f, 1e-300)))
            det = np.ones(f.size, dtype=bool) if lim is None else np.asarray(lim) == 0
            p_out = np.full(f.size, np.nan)
            if det.any():
                q = par[g]
                p_out[det] = outlier_terms(r[det], ln_err[det], w[det], q["s"], q["frac"], q["scale"], q["shift"])[1]
            return np.where(det, r, np.nan), p_out
        point = None
        if self._all_grp is not None and any((self._all_grp == g).any() for g in par):
            n = self._all_t.size
            F = np.empty(n)
            with lock:
                _lib.check(lib.vag_flux_density_batch(h, C.byref(p), 1, self._all_t.ctypes.data_as(_dp), self._all_nu.ctypes.data_as(_dp), n,
                                                      F.ctypes.data_as(_dp)))
            point = with_templates(F, self._all_tmpl, self._ext_kernel)
        out = []
        for g in sorted(par):
            parts = []
            if point is not None and (self._all_grp == g).any():
                sel = self._all_grp == g
                lim = self._all_lim["kind"][sel] if self._all_lim is not None else None
                r, po = rows_of(point[sel], self._all_log_flux[sel], self._all_log_err[sel], self._all_weights[sel], lim, g)
                parts.append((self._all_t[sel], self._all_nu[sel], np.full(int(sel.sum()), -1), r, po))
            for k, bd in enumerate(self._band_obs):
                if bd["noise"] != g:
                    continue
                n = bd["t"].size
                F = np.empty(n)
                with lock:
                    _lib.check(lib.vag_flux_batch(h, C.byref(p), 1, bd["t"].ctypes.data_as(_dp), n, bd["nu_min"], bd["nu_max"],
                                                  bd["num_points"], F.ctypes.data_as(_dp)))
                r, po = rows_of(with_templates(F, bd.get("tmpl"), None), bd["ln_flux"], bd["ln_err"], bd["weights"], bd["lim"], g)
                parts.append((bd["t"], np.full(n, np.nan), np.full(n, k), r, po))
            cols = [np.concatenate(c) if parts else np.array([]) for c in (zip(*parts) if parts else [[]] * 5)]
            out.append(dict(label=labels[g], t=cols[0], nu=cols[1], band=cols[2].astype(np.int64), residual=cols[3], p_out=cols[4]))
        return out

    def count_spectra(self, best_params, param_defs, resolution=None):
        """The expected counts mu [n][C] of every count-spectrum group at a point of sampler space: a list of float64 arrays, one per
        group.  Each group is one vag_flux_density_batch request at its n_samples J points (t_sample_s, nu_j), s outer, and
        fold_expected on the result with the sample's N_H -- the likelihood's own request and arithmetic (its flux may differ from
        this call's in the last bits)."""
        p, _ = self._params_at(best_params, param_defs, resolution)
        spec, _, _ = self.build_spec(param_defs)
        sample = np.asarray(best_params, dtype=np.float64).reshape(-1)
        n_h = spec._fold.n_h_fixed if spec._fold is not None else self.n_h
        for d in range(spec.ndim):
            if spec.slot[d] == _lib.P_N_H:
                n_h = 10.0 ** sample[d] if spec.is_log[d] else sample[d]
        h, lock = get_context(self.device)
        out = []
        for gd in self._fold_obs:
            ns, J = gd["t_sample"].size, gd["nu"].size
            ts, nus = np.ascontiguousarray(np.repeat(gd["t_sample"], J)), np.ascontiguousarray(np.tile(gd["nu"], ns))
            flux = np.empty(ns * J)
            with lock:
                _lib.check(_lib.load().vag_flux_density_batch(h, C.byref(p), 1, ts.ctypes.data_as(_dp), nus.ctypes.data_as(_dp), ns * J,
                                                              flux.ctypes.data_as(_dp)))
            out.append(fold_expected(flux, gd, n_h))
        return out

    def visibilities(self, best_params, param_defs, resolution=None):
        """The model visibilities at the data of every visibility group at a point of sampler space: a list of complex128 arrays,
        one per group, in the order and layout the data were added.  Each group is one Model.sky_visibilities request at the
        group's epochs, frequency and n_az with the walker's pa; the phase of east0 / north0 is applied on the host."""
        spec, _, _ = self.build_spec(param_defs)
        sample = np.asarray(best_params, dtype=np.float64).reshape(-1)
        place = dict(pa=spec._sky.pa_fixed, east0=spec._sky.east0_fixed, north0=spec._sky.north0_fixed) if spec._sky is not None \
            else dict(pa=0.0, east0=0.0, north0=0.0)
        by_slot = {slot: name for name, slot in _lib.SKY_SLOTS.items()}
        for d in range(spec.ndim):
            if spec.slot[d] in by_slot:
                place[by_slot[spec.slot[d]]] = 10.0 ** sample[d] if spec.is_log[d] else sample[d]
        model = self.model(best_params, param_defs, resolution)
        out = []
        for vd in self._vis_obs:
            first, ne = vd["first"], vd["t"].size
            nbl = int(np.diff(first).max())
            u, v = np.zeros((1, ne, nbl)), np.zeros((1, ne, nbl))  # the ragged epochs padded to a rectangle
            for e in range(ne):
                n = first[e + 1] - first[e]
                u[0, e, :n], v[0, e, :n] = vd["u"][first[e]:first[e + 1]], vd["v"][first[e]:first[e + 1]]
            rect = model.sky_visibilities(vd["t"], np.array([vd["nu"]]), u, v, pa=place["pa"], n_az=vd["n_az"])[0]
            flat = np.concatenate([rect[e, :first[e + 1] - first[e]] for e in range(ne)])
            out.append(flat * np.exp(-2j * np.pi * (vd["u"] * place["east0"] + vd["v"] * place["north0"])))
        return out

    # fitting/params.py validate_parameters: the checks that do not depend on the sampler
    def validate_parameters(self, param_defs: Sequence[ParamDef]) -> None:
        names = [pd.name for pd in param_defs]
        if len(set(names)) != len(names):
            raise ValueError("duplicate parameter names")
        for pd in param_defs:
            if pd.name not in ("A_V", "N_H") and pd.name not in _lib.PARAM_SLOTS and pd.name not in _lib.SKY_SLOTS and pd.name not in _lib.POL_SLOTS \
                    and not pd.name.startswith(_lib.NOISE_PREFIX) and not pd.name.startswith(_lib.TMPL_PREFIX) \
                    and not pd.name.startswith(tuple(_lib.ROBUST_PREFIXES)):
                # (sys_<label>, amp_<name>, out_*_<label>: _check_noise_parameters, _check_template_parameters, _check_outlier_parameters below)
                raise ValueError(f"parameter {pd.name} is not accepted by the accelerated path")
            if pd.scale is Scale.fixed:
                continue
            if not (np.isfinite(pd.lower) and np.isfinite(pd.upper) and pd.lower < pd.upper):
                raise ValueError(f"{pd.name}: need finite lower < upper, got [{pd.lower}, {pd.upper}]")
            if pd.scale is Scale.log and pd.lower <= 0:
                raise ValueError(f"{pd.name}: log-scale parameters need lower > 0")
        if "A_V" in names and self.extinction is None:
            raise ValueError("A_V needs Fitter(extinction=...)")
        self._check_pol_parameters(names)
        self._check_noise_parameters(param_defs)
        self._check_outlier_parameters(param_defs)
        self._check_template_parameters(param_defs)
        self._check_n_h_parameter(param_defs)

    def _params_at(self, sample, param_defs, resolution=None):
        """vag_model_params and A_V of one point of sampler space (the transformer of fitting/utils.py:110-135)."""
        spec, _, _ = self.build_spec(param_defs)
        sample = np.asarray(sample, dtype=np.float64).reshape(-1)
        if sample.size != spec.ndim:
            raise ValueError(f"expected {spec.ndim} free parameters, got {sample.size}")
        p = _lib.ModelParams.from_buffer_copy(bytes(spec.base))
        fields = (C.c_double * 40).from_address(C.addressof(p) + _lib.ModelParams.theta_c.offset)
        a_v = spec.a_v_fixed
        for d in range(spec.ndim):
            val = 10.0 ** sample[d] if spec.is_log[d] else sample[d]
            if spec.slot[d] == _lib.P_A_V:
                a_v = val
            elif spec.slot[d] > _lib.P_A_V:  # (the sky placement: not a Model field)
                continue
            else:
                fields[spec.slot[d]] = val
        if resolution is not None:
            p.phi_resol, p.theta_resol, p.t_resol = (float(x) for x in resolution)
        return p, float(a_v)

    # fitter.py:1089-1099
    def model(self, best_params, param_defs, resolution=None):
        """The underlying Model at a point of sampler space (no extinction applied)."""
        from .model import Model
        return Model.from_params(self._params_at(best_params, param_defs, resolution)[0], device=self.device)

    # fitter.py:779-804
    def flux_density_grid(self, best_params, t, nu, param_defs, resolution=None):
        """FluxDict on a (t, nu) grid at a point of sampler space; host-galaxy extinction (Fitter(extinction=...), A_V != 0) is
        applied per frequency to every component, like the fitter's own chi-squared path."""
        from .model import Model, FluxDict
        p, a_v = self._params_at(best_params, param_defs, resolution)
        res = Model.from_params(p, device=self.device).flux_density_grid(t, nu)
        if self.extinction is None or a_v == 0.0:
            return res
        lam_rest_cm = (2.99792458e10 / np.asarray(nu, dtype=np.float64)) / (1.0 + self.z)
        att = np.exp(-a_v * 0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64))[:, None]
        comps = [c * att if np.ndim(c) == 2 else None for c in (res.fwd.sync, res.fwd.ssc, res.rvs.sync, res.rvs.ssc)]
        return FluxDict(*comps)

    # fitter.py:806-833
    def flux(self, best_params, t, band, param_defs, num_points=5, resolution=None):
        """Band-integrated flux [erg/cm^2/s] over band = (nu_min, nu_max) at a point of sampler space (no extinction)."""
        nu_min, nu_max = band
        return self.model(best_params, param_defs, resolution).flux(t, nu_min, nu_max, num_points)

    def predict(self, samples, param_defs, t, nu, quantiles=(0.16, 0.5, 0.84), draws=None, seed=0, resolution=None,
                return_draws=False):
        """Posterior-predictive quantile bands of the flux density on the grid t[nt] x nu[nnu], in ONE device call
        (vag_predict_bands_dev; INTEGRATION.md "Posterior-predictive bands"): every drawn row of ``samples`` [N, ndim] (sampler space:
        ``fit()["samples"]`` fits directly) becomes a model, the models run as one batch, each draw's fluxes take the fitter's
        extinction law at ``nu`` with the draw's own A_V (as flux_density_grid applies it), and ``quantiles`` are taken over the valid
        draws at every (nu, t) by the definition of sampling.column_quantiles.  ``draws=None`` uses every row; ``draws=k`` the rows
        np.sort(np.random.default_rng(seed).choice(N, k, replace=False)).  ``resolution`` overrides the fitter's (phi, theta, t)
        resolution.  A draw the engine cannot evaluate (or with a parameter that is not finite) is invalid and left out.  Returns a
        sampling.Prediction; ``return_draws`` adds the draws' own fluxes [S, nnu, nt]."""
        import torch
        from . import sampling
        spec, _, _ = self.build_spec(param_defs)
        samples = np.asarray(samples, dtype=np.float64)
        if samples.ndim != 2 or samples.shape[1] != spec.ndim:
            raise ValueError(f"predict: samples must be [N, {spec.ndim}] in sampler space, got shape {samples.shape}")
        n_rows = samples.shape[0]
        q = sampling._quantile_levels(quantiles)
        if draws is None:
            if n_rows > sampling.PREDICT_MAX_DRAWS:
                raise ValueError(f"predict: {n_rows} samples exceed the {sampling.PREDICT_MAX_DRAWS} draws of one call; pass draws= "
                                 "to take a random subset")
            index = np.arange(n_rows)
        else:
            if int(draws) != draws or draws < 1:
                raise ValueError(f"predict: draws= must be a whole number >= 1, got {draws}")
            if draws > n_rows:
                raise ValueError(f"predict: draws={draws} exceeds the {n_rows} rows of samples")
            if draws > sampling.PREDICT_MAX_DRAWS:
                raise ValueError(f"predict: draws={draws} exceeds the {sampling.PREDICT_MAX_DRAWS} draws of one call")
            index = np.sort(np.random.default_rng(seed).choice(n_rows, int(draws), replace=False))
        if index.size < 1:
            raise ValueError("predict: samples holds no row")
        t = np.ascontiguousarray(t, dtype=np.float64)
        nu = np.ascontiguousarray(nu, dtype=np.float64)
        if t.ndim != 1 or t.size < 1 or not np.all(np.isfinite(t) & (t > 0)) or np.any(np.diff(t) < 0):
            raise ValueError("predict: t must be a non-empty 1-D array of positive finite times in ascending order")
        if nu.ndim != 1 or nu.size < 1 or not np.all(np.isfinite(nu) & (nu > 0)):
            raise ValueError("predict: nu must be a non-empty 1-D array of positive finite frequencies")
        S, nt, nnu = int(index.size), int(t.size), int(nu.size)
        if S * nt * nnu > sampling.PREDICT_MAX_VALUES:
            raise ValueError(f"predict: {S} draws on a {nnu} x {nt} grid exceed the {sampling.PREDICT_MAX_VALUES} values of one call; "
                             "pass a smaller draws= or a coarser grid")
        if resolution is not None:
            spec.base.phi_resol, spec.base.theta_resol, spec.base.t_resol = (float(x) for x in resolution)
        ext = None
        if self.extinction is not None:  # the law at nu, at the fitter's z, as flux_density_grid takes it
            lam_rest_cm = (2.99792458e10 / nu) / (1.0 + self.z)
            ext = np.ascontiguousarray(0.4 * np.log(10.0) * np.asarray(self._k_lambda(lam_rest_cm), dtype=np.float64))
            if ext.shape != nu.shape:
                raise ValueError("predict: the extinction law must return one k(lambda) per frequency")
        lib = _lib.load()
        entry = _lib.predict_entry(lib, "vag_predict_bands_dev")
        h, lock = get_context(self.device)
        dev = torch.device("cuda", self.device)
        qspec = _lib.QuantileSpec(q.size, 0, (C.c_double * 16)(*q.tolist()))
        d_theta = torch.as_tensor(np.ascontiguousarray(samples[index]), device=dev)
        d_t, d_nu = torch.as_tensor(t, device=dev), torch.as_tensor(nu, device=dev)
        d_ext = torch.as_tensor(ext, device=dev) if ext is not None else None
        d_bands = torch.empty((q.size, nnu, nt), dtype=torch.float64, device=dev)
        d_draws = torch.empty((S, nnu, nt), dtype=torch.float64, device=dev) if return_draws else None
        d_valid = torch.empty((S,), dtype=torch.int32, device=dev)
        d_n = torch.empty((1,), dtype=torch.int32, device=dev)
        on_current_stream(lib, h, lock, dev, lambda: _lib.check(entry(
            h, C.byref(spec), d_theta.data_ptr(), S, spec.ndim, d_t.data_ptr(), nt, d_nu.data_ptr(), nnu,
            d_ext.data_ptr() if d_ext is not None else None, C.byref(qspec), d_bands.data_ptr(),
            d_draws.data_ptr() if return_draws else None, d_valid.data_ptr(), d_n.data_ptr())))
        return sampling.Prediction(q, d_bands.cpu().numpy(), int(d_n.cpu().numpy()[0]), d_valid.cpu().numpy() != 0, index, t, nu,
                                   d_draws.cpu().numpy() if return_draws else None)

    # fitter.py:545-674 (the emcee branch; the stretch-move sampler of vegasafterglow_amd.sampling needs no third-party package)
    def fit(self, param_defs, nwalkers=None, nsteps=1000, nburn=0, seed=0, sampler="host", **kw):
        """sampling.fit on this fitter.  ``sampler="host"``: the numpy stretch move around one device call per half-step;
        ``sampler="device"``: the whole run on the device (sampling.run_stretch_move_device, or with ``moves="reference"`` or a
        sequence of (name, weight) sampling.run_moves_device: the DE and snooker moves of the reference); ``sampler="tempered"``: parallel
        tempering on the device (sampling.run_tempered_device; ``ntemps``, ``beta_min``, ``prior_rung`` shape the ladder, `nwalkers`
        is per temperature), which also returns the evidence by thermodynamic integration.  Every sampler reports "tau" and
        "tau_reliable", the autocorrelation time of each parameter after the burn-in; ``converge=sampling.Convergence(...)`` makes
        `nsteps` a maximum for the device samplers and stops the run when tau has settled (sampling.fit).

        ``sampler="nested"``: nested sampling on the device (sampling.run_nested_device) with `nwalkers` live points, `nsteps` the
        maximum number of iterations, ``dlogz=0.1`` the stopping rule, ``walk=None`` the constrained steps per iteration and
        ``priors=None`` the priors.  It returns the weighted samples, "log_evidence" with its error sqrt(H / N) from the run itself,
        "information", "prior_fraction" and "log_prior_mass".  "log_evidence" includes ln prior_fraction (points where the model does
        not evaluate count as L = 0); the tempered number excludes it; both are relative to the prior mass inside the boxes, which
        is "log_prior_mass" (sampling.fit)."""
        from . import sampling
        self.validate_parameters(param_defs)
        ndim = sum(1 for pd in param_defs if pd.scale is not Scale.fixed)
        return sampling.fit(self, param_defs, nwalkers=nwalkers or max(2 * ndim + 2, 32), nsteps=nsteps, nburn=nburn, seed=seed,
                            sampler=sampler, **kw)

    def loglike_batch(self, samples, param_defs):
        """ln L for each row of samples[nb, ndim] (one batched device call)."""
        spec, _, _ = self.build_spec(param_defs)
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        if samples.ndim != 2 or samples.shape[1] != spec.ndim:
            raise ValueError("samples must be [nb, ndim]")
        return self._device_loglike(spec, samples)

    def device_evaluator(self, param_defs, priors=None, use_priors=False, context=None):
        """eval_dev(theta) -> (values, costs) for vegasafterglow_amd.dist.WalkerSharder: theta is a float64 torch tensor [k, ndim]
        on this fitter's GPU; values = ln L (use_priors=False) or ln L + ln prior with the bounds mask (use_priors=True),
        costs = the engine's per-walker cell counts -- both float64[k] tensors on the device.  The call runs on torch's current
        stream through vag_loglike_batch_dev: nothing crosses PCIe.  Priors that only exist as host objects are not accepted
        here (the device path must be self-contained)."""
        import torch
        spec, _, _ = self.build_spec(param_defs, priors=priors, use_priors=use_priors)
        self._refuse_host_priors(param_defs, "device_evaluator")
        lib = _lib.load()
        if context is None:
            h, lock = get_context(self.device)
        else:
            h, lock = context
        dev = torch.device("cuda", self.device)
        keep = [spec]  # the spec's arrays are owned by this Fitter; the struct itself by this closure

        def _on_current_stream(fn):
            return on_current_stream(lib, h, lock, dev, fn)

        def eval_dev(theta, want_costs=True):
            theta = theta.contiguous()
            k = theta.shape[0]
            values = torch.empty((k,), dtype=torch.float64, device=dev)
            costs = torch.empty((k,), dtype=torch.float64, device=dev) if want_costs else None

            def run():
                ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
                # the widest entry point: with a block absent (None) it is the narrower entry point, bit for bit
                fn, fold = _widest_entry(lib, keep[0], "_dev")  # (fold: the trailing specs -- the fold block, the templates, the correlated groups)
                _lib.check(fn(h, C.byref(keep[0]), ref(keep[0]._sky), ref(keep[0]._vis), ref(keep[0]._pol), ref(keep[0]._lim),
                              ref(keep[0]._noise), ref(keep[0]._counts), ref(keep[0]._index), *fold, theta.data_ptr(), k, keep[0].ndim,
                              values.data_ptr()))
                if want_costs:  # (one more launch: only a sharder that deals by cost asks for it)
                    _lib.check(lib.vag_last_model_costs_dev(h, k, costs.data_ptr()))
            _on_current_stream(run)
            return values, costs
        eval_dev.optional_costs = True
        from .dist import DATA_KINDS
        for attr, has, _ in DATA_KINDS:
            setattr(eval_dev, has, getattr(spec, attr) is not None)
        eval_dev.has_centroids = eval_dev.has_centroids and spec._sky.n_groups > 0  # (n_groups = 0: the fixed placement alone)

        class _Native:
            """The engine's own sharded call for dist.WalkerSharder: deal + this rank's block, then the scatter after the
            all-gather (vag_loglike_shard_begin_dev / vag_loglike_shard_end_dev); no host work besides the launches."""
            parts = (lib, h, lock, keep)
            check = staticmethod(_lib.check)

            @staticmethod
            def shard(theta_all, nb, rank, world, block):
                """Returns the ticket that names this call in flight; finish() takes it (ABI v13)."""
                for attr, _, why in reversed(DATA_KINDS):
                    if getattr(keep[0], attr) is not None:
                        raise NotImplementedError(why)
                ticket = C.c_uint64(0)
                _on_current_stream(lambda: _lib.check(lib.vag_loglike_shard_begin_dev(
                    h, C.byref(keep[0]), theta_all.data_ptr(), nb, keep[0].ndim, rank, world, block.data_ptr(), C.byref(ticket))))
                return ticket.value

            @staticmethod
            def finish(ticket, gathered, nb, world, out):
                _on_current_stream(lambda: _lib.check(lib.vag_loglike_shard_end_dev(h, ticket, gathered.data_ptr(), nb, world, out.data_ptr())))

            @staticmethod
            def state(nb, world, per):
                tab = torch.empty((world * per,), dtype=torch.int32, device=dev)
                cost = torch.empty((nb,), dtype=torch.float64, device=dev)
                _on_current_stream(lambda: _lib.check(lib.vag_loglike_shard_state_dev(h, nb, world, tab.data_ptr(), cost.data_ptr())))
                return tab.cpu().numpy().astype(np.int64).reshape(world, per), cost.cpu().numpy()

        _Native.lock = lock  # dist.WalkerSharder takes it around shard() and around finish() (not across the all-gather between them)
        eval_dev.native = _Native
        return eval_dev

    def _refuse_host_priors(self, param_defs, who):
        """After build_spec: a path that must be self-contained on the device takes no prior that only exists as a host object."""
        if self._host_priors:
            free = [pd.name for pd in param_defs if pd.scale is not Scale.fixed]
            raise ValueError(f"{who}: only Uniform / Gaussian / LogUniform priors (or their tuple forms) run on the device; "
                             f"got host-only priors for {[free[d] for d, _ in self._host_priors]}")

    @staticmethod
    def _log_plan_warnings(plan, nb):
        if plan.n_models_capacity:
            # never silent: these walkers were NOT evaluated (their adaptive grid exceeds the engine's static limits)
            logger.warning("%d of %d walkers exceeded the engine grid limits and were assigned -inf", plan.n_models_capacity, nb)
        if plan.n_walkers_ssc_failed:
            logger.warning("%d of %d walkers had SSC tables outside the engine's capacity and were assigned -inf",
                           plan.n_walkers_ssc_failed, nb)

    def _device_loglike(self, spec, samples):
        out = np.empty(samples.shape[0])
        h, lock = get_context(self.device)
        plan = _lib.Plan()
        with lock:
            ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
            # the widest entry point: with a block absent (None) it is the narrower entry point, bit for bit
            fn, fold = _widest_entry(_lib.load(), spec, "")
            _lib.check(fn(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise),
                          ref(spec._counts), ref(spec._index), *fold, samples.ctypes.data_as(_dp), samples.shape[0], spec.ndim,
                          out.ctypes.data_as(_dp)))
            _lib.load().vag_last_plan(h, C.byref(plan))
        self._log_plan_warnings(plan, samples.shape[0])
        self.last_plan = plan
        return out

    def log_prob_batch(self, samples, param_defs, priors=None):
        """log_prob_batch of fitting/samplers.py:72-91 in ONE device call: walkers outside the ParamDef bounds are not evaluated
        and score -inf, the others ln L + sum ln prior.  ``priors`` maps parameter names to priors acting on the SAMPLER-space
        value: objects shaped like bilby.core.prior.Uniform / Gaussian / LogUniform (or ("gaussian", mu, sigma),
        ("log_uniform", minimum, maximum), ("uniform",)) run on the device; any other object with ``ln_prob`` is added on the host.
        Parameters without an entry get Uniform(lower, upper) (params.py:209-227)."""
        spec, _, _ = self.build_spec(param_defs, priors=priors, use_priors=True)
        samples = np.ascontiguousarray(np.atleast_2d(np.asarray(samples, dtype=np.float64)))
        if samples.shape[1] != spec.ndim:
            raise ValueError("samples must be [nb, ndim]")
        out = self._device_loglike(spec, samples)
        for d, prior in self._host_priors:
            out = out + np.asarray(prior.ln_prob(samples[:, d]), dtype=np.float64)
        out[~np.isfinite(out)] = -np.inf
        return out

    def log_like_and_prior_batch(self, samples, param_defs, priors=None):
        """(ln L, ln prior) of each row of samples[nb, ndim], apart, in ONE device call (vag_loglike_split_dev): what tempering
        needs, which scales ln L alone.  ln prior is the sum of the priors with the bounds mask, as in log_prob_batch (host-only
        priors are added on the host); ln L is -inf for a walker that was not evaluated, one outside the bounds included.
        ln L + ln prior equals log_prob_batch to the bit wherever that is finite."""
        import torch
        from . import sampling
        spec, _, _ = self.build_spec(param_defs, priors=priors, use_priors=True)
        samples = np.ascontiguousarray(np.atleast_2d(np.asarray(samples, dtype=np.float64)))
        if samples.shape[1] != spec.ndim:
            raise ValueError("samples must be [nb, ndim]")
        dev = torch.device("cuda", self.device)
        theta = torch.from_numpy(samples).to(dev)
        lnl = torch.empty((samples.shape[0],), dtype=torch.float64, device=dev)
        lnprior = torch.empty_like(lnl)
        sampling.loglike_split_device(self, spec, theta, lnl, lnprior)
        plan = _lib.Plan()
        h, lock = get_context(self.device)
        with lock:
            _lib.load().vag_last_plan(h, C.byref(plan))
        self._log_plan_warnings(plan, samples.shape[0])
        self.last_plan = plan
        lnl, lnprior = lnl.cpu().numpy(), lnprior.cpu().numpy()
        for d, prior in self._host_priors:
            lnprior = lnprior + np.asarray(prior.ln_prob(samples[:, d]), dtype=np.float64)
        return lnl, lnprior

    def make_log_prob_batch(self, param_defs, loglike_fn=None, priors=None):
        """log_prob_batch(samples) of fitting/samplers.py:72-91: out-of-bounds -> -inf; otherwise ln L + sum ln prior, evaluated
        by the device in one call (Fitter.log_prob_batch).  ``loglike_fn`` substitutes an evaluator of ln L alone (e.g. one that
        shards walkers over ranks); the bounds mask and EVERY prior of ``priors`` are then applied here on the host
        (host_ln_prior: the same closed forms as the device, or the prior object's ln_prob)."""
        if loglike_fn is None:
            return lambda samples: self.log_prob_batch(samples, param_defs, priors=priors)
        _, lower, upper = self.build_spec(param_defs, priors=priors, use_priors=True)
        prior_specs = list(self._prior_specs)
        fn = loglike_fn

        def log_prob_batch(samples):
            samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
            ln_prior = host_ln_prior(samples, lower, upper, prior_specs)  # -inf outside the bounds or a prior's support
            log_probs = np.full(samples.shape[0], -np.inf)
            idx = np.where(ln_prior > -np.inf)[0]
            if idx.size:
                ll = np.asarray(fn(samples[idx]), dtype=np.float64)
                ll[~np.isfinite(ll)] = -np.inf
                log_probs[idx] = ll + ln_prior[idx]
            return log_probs

        return log_prob_batch
