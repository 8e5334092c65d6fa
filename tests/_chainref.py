"""Shared by the chain-autocorrelation tests (checker only): AR(1) test chains with means and widths like the C4 parameters, and the
extended-precision reference of INTEGRATION.md "Chain autocorrelation" -- np.longdouble direct sums, written here and sharing no code
with the package."""
import numpy as np

# mean, width and AR(1) coefficient per parameter: log10 E, Gamma0, theta_c, p, log10 eps_B, ...; the fifth mixes too slowly for its
# window to fit into the default lag range of a 1500-row chain (for most seeds)
PARAMETERS = ((52.4, 0.1, 0.5), (500.0, 40.0, 0.8), (0.07, 0.01, 0.9), (2.3, 0.05, 0.0), (-1.5, 0.3, 0.95), (0.3, 0.05, 0.7),
              (-2.0, 0.4, 0.6), (1.2, 0.2, 0.85))


def ar1_chain(n, nwalkers, ndim, seed, parameters=PARAMETERS):
    """chain[n, W, D]: parameter d of every walker an AR(1) series with coefficient phi_d, started in its stationary law, scaled and
    shifted to the mean and width of PARAMETERS[d]."""
    rng = np.random.default_rng(seed)
    mean, width, phi = (np.array([p[k] for p in parameters[:ndim]]) for k in range(3))
    x = np.empty((n, nwalkers, ndim))
    noise = rng.standard_normal((n, nwalkers, ndim))
    x[0] = noise[0] / np.sqrt(1.0 - phi ** 2)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + noise[t]
    return mean + width * np.sqrt(1.0 - phi ** 2) * x


def exact_tau(phi):
    return (1.0 + phi) / (1.0 - phi)


class Reference:
    """rho[L + 1, D] (np.longdouble), tau[D], window[D] and margin[D] of chain[n, W, D]: margin is the smallest |M - c tau(M)| over
    the M up to the window (up to L where there is none), the distance of the nearest window decision from its threshold."""

    def __init__(self, chain, c, max_lag):
        x = np.asarray(chain, dtype=np.longdouble)
        n = x.shape[0]
        y = x - x.sum(axis=0) / n
        pooled = np.array([(y[:n - lag] * y[lag:]).sum(axis=(0, 1)) for lag in range(max_lag + 1)])
        with np.errstate(invalid="ignore", divide="ignore"):
            self.rho = pooled / pooled[0]
        taus = 2 * np.cumsum(self.rho, axis=0) - 1
        gap = np.arange(max_lag + 1, dtype=np.longdouble)[:, None] - np.longdouble(c) * taus
        ndim = x.shape[2]
        self.tau, self.window, self.margin = np.empty(ndim), np.empty(ndim, dtype=np.int32), np.empty(ndim)
        for d in range(ndim):
            ok = np.nonzero(gap[:, d] >= 0)[0]
            last = ok[0] if ok.size else max_lag
            self.window[d] = ok[0] if ok.size else -1
            self.tau[d] = float(taus[last, d])
            self.margin[d] = float(np.abs(gap[:last + 1, d]).min())
        self.pooled0 = pooled[0].astype(np.float64)


def rho_bound(n):
    """|rho - reference| of a float64 estimate: an fma chain of n terms each bounded by C(0), the division, and slack"""
    return 8.0 * n * 2.0 ** -53
