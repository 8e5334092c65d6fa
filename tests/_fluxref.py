"""Extended-precision reference of the synchrotron flux stage alone (tests/test_flux_stage_host.py, tests/test_flux_stage.py).

A plain numpy.longdouble restatement (mpmath through _mathref's backends where longdouble is no wider than a double) of what the
reference does between the solved shock and the flux: Observer::observe (oracle/vag_oracle.c observe(): phi bin widths, theta-bin solid
angles, cos_v, Doppler factor and observer time per cell, lg2_geom = log2(dOmega r^2) + 3 lg2_doppler, with and without lateral
spreading), the spectrum of every lattice node (_mathref.photons_build / log2_I_nu), and specific_flux (grid form, iterate_to),
specific_flux_series (series form, iterate_through) and the band form (compute_boole_weights over the grid form).

Its inputs are the arrays a details call returns for ONE model -- phi, theta, t_src, r, Gamma, the polar angle per cell, nu_m, nu_c,
nu_a, nu_M, I_nu_max -- plus z, lumi_dist, theta_obs and p.  It imports neither the library nor the oracle, and it computes the lattice
itself.  Everything is in the engine's code units (_mathref's U_* constants); `cells_from_cgs` / `cells_from_oracle` bring the two
producers' details there.

Rules ported as written: a row contributes from its first node on; a bracket whose slope is not finite contributes nothing; the grid
form puts a time into the bracket t_k <= t < t_k+1 (a time on the last node is outside), the series form into t_k < t <= t_k+1 (the
last node is inside).  The interpolant is continuous across interior nodes, so the bracket chosen there does not matter; at a row's
first and last node it does, and a double computation may land on either side.  For requested times within EDGE_ULPS ulp (of log2 t)
of such a node the result therefore carries both decisions (`Flux.alt`), and `Flux.nearest` accepts the nearer one -- as `_mathref`
treats its thresholds (`side=`).  An "ulp" of a node here is what one rounding does to a DOUBLE computation of that node, whoever makes
it: spacing(log2 t_obs) plus the rounding of the time itself, log2(e) eps (t + 3 r / c)(1 + z) / t_obs (`lattice`'s lg2_t_ulp).  The
second part matters where t_obs is the small difference of t and r cos_v / c: a head-on cell of Lorentz factor 300 has
r / (c t_obs) ~ 2e5, so no double lattice places its nodes better than ~1e-11, and a request a few ulp from the device's own node
(tests/test_flux_stage.py) lies on either side of the extended-precision node.

The spectrum's own thresholds (the +-20 softplus cuts, log2_x_far, the nu_M cut) are `_mathref`'s: `FluxStage.all_sides` evaluates a
request under side = None, -1, +1 and `FluxSides.nearest` accepts each slot at the nearest of the three.

Not covered: SSC components (their tables are not in the details), non-axisymmetric jets, exposure averaging.
"""
import itertools

import numpy as np

import _mathref as mr

U_HZ = 1 / mr.U_SEC
U_ERG = mr.U_G * mr.U_CM * mr.U_CM / mr.U_SEC / mr.U_SEC
U_CM2 = mr.U_CM * mr.U_CM
U_FLUX_CGS = U_ERG / U_CM2 / mr.U_SEC
U_FLUX_DEN_CGS = U_ERG / U_CM2 / mr.U_SEC / U_HZ
EDGE_ULPS = 4
RAD_NAMES = ("nu_m", "nu_c", "nu_a", "nu_M", "I_nu_max")


def _fn(B, name):
    """sin / cos of the backend (numpy for longdouble, mpmath element-wise)."""
    if B is mr.LD:
        return getattr(np, name)
    return np.frompyfunc(getattr(mr.mpmath, name), 1, 1)


def cells_from_cgs(shock, rad=None):
    """Code-unit cells from a product details dictionary (cgs / Hz): `shock` gives phi, theta, t_src, r, Gamma, theta_cell and shape,
    `rad` (default: the same) the five radiation arrays.  The reverse shock radiates on the forward shock's lattice, so its cells are
    cells_from_cgs(forward details, reverse details)."""
    rad = shock if rad is None else rad
    c = dict(phi=np.asarray(shock["phi"], dtype=np.float64), theta=np.asarray(shock["theta"], dtype=np.float64),
             t=np.asarray(shock["t_src"], dtype=np.float64) * mr.U_SEC, r=np.asarray(shock["r"], dtype=np.float64) * mr.U_CM,
             Gamma=np.asarray(shock["Gamma"], dtype=np.float64), theta_cell=np.asarray(shock["theta_cell"], dtype=np.float64),
             phi_mirrored=int(shock["shape"]["phi_mirrored"]))
    for n in RAD_NAMES[:4]:
        c[n] = np.asarray(rad[n], dtype=np.float64) * U_HZ
    c["I_nu_max"] = np.asarray(rad["I_nu_max"], dtype=np.float64) * U_FLUX_DEN_CGS
    return c


def cells_from_oracle(shock, rad=None):
    """The same from the oracle's details: its r and t_src are in cgs, its radiation arrays already in code units."""
    rad = shock if rad is None else rad
    c = cells_from_cgs(shock, dict(nu_m=0, nu_c=0, nu_a=0, nu_M=0, I_nu_max=0))
    for n in RAD_NAMES:
        c[n] = np.asarray(rad[n], dtype=np.float64)
    return c


# ---- geometry: observe() ----
def phi_widths(phi, n_phi_eff, mirrored, B=mr.DEFAULT):
    """The phi bin widths: the on-axis single bin, mirrored bins (half circle, counted twice), plain bins."""
    if n_phi_eff == 1:
        return B.arr([2 * mr.C_PI])
    ph = B.arr(phi[:n_phi_eff])
    last = n_phi_eff - 1
    out = []
    for i in range(n_phi_eff):
        if mirrored:
            left = (ph[i - 1] + ph[i]) / 2 if i > 0 else B.const(0.0)
            right = (ph[i] + ph[i + 1]) / 2 if i < last else B.const(mr.C_PI)
            out.append(2 * (right - left))
        else:
            out.append((ph[min(i + 1, last)] - ph[max(i - 1, 0)]) / 2)
    return np.array(out, dtype=ph.dtype)


def _interp_theta(t_nb, th_nb, t_target):
    """INTERP_THETA_: the neighbouring row's polar angle at a cell's engine time (linear; its last node's beyond the row's end; the
    first bracket extrapolated before its first node)."""
    nt = t_nb.size
    cnt = np.array([int(np.sum(np.asarray(t_nb < tt, dtype=bool))) for tt in t_target])  # nodes strictly before the target
    out = np.empty_like(th_nb)
    for k, c in enumerate(cnt):
        h = max(c - 1, 0)
        if h + 1 >= nt:
            out[k] = th_nb[nt - 1]
        else:
            w = (t_target[k] - t_nb[h]) / (t_nb[h + 1] - t_nb[h])
            out[k] = th_nb[h] + w * (th_nb[h + 1] - th_nb[h])
    return out


def lattice(cells, z, theta_obs, spreading, B=mr.DEFAULT):
    """The equal-arrival-time lattice: lg2_t, lg2_doppler, lg2_geom, each [n_phi_eff][n_theta][n_t] (backend values)."""
    sin, cos = _fn(B, "sin"), _fn(B, "cos")
    t, r, G = B.arr(cells["t"]), B.arr(cells["r"]), B.arr(cells["Gamma"])
    nth, nt = t.shape
    n_phi_eff = 1 if theta_obs == 0 else cells["phi"].size
    dphi = phi_widths(cells["phi"], n_phi_eff, cells["phi_mirrored"], B)
    obs = B.arr([theta_obs])[0]
    cos_obs, sin_obs = cos(obs), sin(obs)
    one_z = 1 + B.const(z)
    last = nth - 1
    if spreading:
        th = B.arr(cells["theta_cell"])
        dcos = np.empty_like(th)
        for j in range(nth):
            lo = th[j] if j == 0 else (th[j] + _interp_theta(t[j - 1], th[j - 1], t[j])) / 2
            hi = th[j] if j == last else (th[j] + _interp_theta(t[j + 1], th[j + 1], t[j])) / 2
            dcos[j] = cos(hi) - cos(lo)
    else:
        th1 = B.arr(cells["theta"])
        edge = np.empty(nth + 1, dtype=th1.dtype)
        edge[0], edge[nth] = cos(th1[0]), cos(th1[last])
        for j in range(last):
            edge[j + 1] = cos((th1[j] + th1[j + 1]) / 2)
        th = np.repeat(th1[:, None], nt, axis=1)
        dcos = np.repeat((edge[1:] - edge[:-1])[:, None], nt, axis=1)
    st, ct = sin(th), cos(th)
    shape = (n_phi_eff, nth, nt)
    lg2_t, lg2_d, lg2_g = (np.empty(shape, dtype=t.dtype) for _ in range(3))
    for i in range(n_phi_eff):
        cos_phi = cos(B.arr([cells["phi"][i]])[0])
        cos_v = st * cos_phi * sin_obs + ct * cos_obs
        dop = G - B.sqrt((G - 1) * (G + 1)) * cos_v
        lg2_d[i] = -B.log2(dop)
        lg2_t[i] = B.log2((t + (1 - cos_v) * r / B.const(mr.C_C)) * one_z)
        lg2_g[i] = B.log2(np.abs(dcos * dphi[i]) * r * r) + 3 * lg2_d[i]
    with np.errstate(all="ignore"):
        t_obs = np.exp2(mr.to_float(lg2_t))
        eps = np.finfo(np.float64).eps
        ulp = np.spacing(np.abs(mr.to_float(lg2_t))) + mr.LOG2E * eps * (mr.to_float(t) + 3 * mr.to_float(r) / mr.C_C)[None] * (1 + z) / t_obs
    return dict(lg2_t=lg2_t, lg2_doppler=lg2_d, lg2_geom=lg2_g, lg2_t_ulp=ulp)


# ---- the boundary spectra, the interpolation and the sum ----
class Flux:
    """A reference flux: `value` (every bracket decided exactly) and, per slot that sits within EDGE_ULPS ulp of some row's first or
    last node, the terms those rows add or remove when decided the other way (`alt`: flat slot index -> list of signed terms);
    `terms`, where asked for, the contribution of every row [n_phi_eff][n_theta] + value.shape."""

    def __init__(self, value, alt, terms=None):
        self.value, self.alt, self.terms = value, alt, terms

    def candidates(self, q):
        d = self.alt.get(q, [])
        assert len(d) <= 8, "more than 8 rows have an edge node at one requested time"
        base = self.value.ravel()[q]
        return [base + sum(c) for n in range(len(d) + 1) for c in itertools.combinations(d, n)]

    def nearest(self, got):
        """The reference as longdouble, each edge slot at the candidate nearest to `got`."""
        ref = mr.to_ld(self.value).copy()
        g = np.asarray(got).ravel()
        flat = ref.reshape(-1)
        for q in self.alt:
            cand = [mr.to_ld(np.array([c]))[0] for c in self.candidates(q)]
            flat[q] = min(cand, key=lambda c: abs(c - np.longdouble(g[q])))
        return flat.reshape(ref.shape)


class FluxSides:
    """One request under the three decisions of the spectrum's own thresholds (_mathref's side = None, -1, +1): a double evaluation
    within THRESH_TOL of a threshold matches one of them, so every slot is accepted at the nearest."""

    def __init__(self, fluxes):
        self.fluxes, self.value, self.alt = fluxes, fluxes[0].value, fluxes[0].alt

    def nearest(self, got):
        cand = np.stack([f.nearest(got) for f in self.fluxes])
        pick = np.argmin(np.abs(cand - np.asarray(got).astype(np.longdouble)[None]), axis=0)
        return np.take_along_axis(cand, pick[None], axis=0)[0]


def _brackets(lg2_t, lg2_t_ulp, T, through):
    """For every row [n_phi_eff][n_theta] and request time T [n]: the bracket's lower node k (clipped into the row), `inside` (the
    exact decision: iterate_to puts T into t_k <= T < t_k+1, iterate_through into t_k < T <= t_k+1 with the first node included) and
    `edge` (T within EDGE_ULPS ulp of the row's first or last node)."""
    npe, nth, K = lg2_t.shape
    k = np.zeros((npe, nth, T.size), dtype=np.int64)
    inside = np.zeros(k.shape, dtype=bool)
    edge = np.zeros(k.shape, dtype=bool)
    Tf = mr.to_float(T)
    for i in range(npe):
        for j in range(nth):
            t_row = lg2_t[i, j]
            assert np.all(np.asarray(t_row[1:] >= t_row[:-1], dtype=bool)), f"row ({i}, {j}): observer times not ascending"
            if through:
                k[i, j] = np.searchsorted(t_row, T, side="left") - 1
                inside[i, j] = np.asarray(T >= t_row[0], dtype=bool) & np.asarray(T <= t_row[K - 1], dtype=bool)
            else:
                k[i, j] = np.searchsorted(t_row, T, side="right") - 1
                inside[i, j] = np.asarray(T >= t_row[0], dtype=bool) & np.asarray(T < t_row[K - 1], dtype=bool)
            for kn in (0, K - 1):
                edge[i, j] |= np.abs(Tf - float(t_row[kn])) <= EDGE_ULPS * lg2_t_ulp[i, j, kn]
    return np.clip(k, 0, K - 2), inside, edge


def _norm(z, lumi_dist, B):
    d = B.arr([np.float64(lumi_dist) * mr.U_CM])[0]
    return (1 + B.const(z)) / (d * d)


class FluxStage:
    """The flux stage of one model (one shock's radiation on the forward shock's lattice)."""

    def __init__(self, cells, p, z, lumi_dist, theta_obs, spreading=False, B=mr.DEFAULT):
        self.cells, self.p, self.z, self.lumi_dist, self.B = cells, float(p), float(z), float(lumi_dist), B
        self.lat = lattice(cells, z, theta_obs, spreading, B)
        self.shape = self.lat["lg2_t"].shape
        self._ph = {}
        self.skip_rows = ()  # (phi, theta) rows left out of every sum, and an offset on one node's lg2_geom: what the sensitivity checks of
        self.geom_shift = None  # tests/test_flux_stage_host.py turn on: ((i, j, k), delta)

    def photons(self, side):
        """_mathref.photons_build of every cell [n_theta][n_t], per decision of the spectrum's own thresholds (None, -1, +1)."""
        if side not in self._ph:
            with np.errstate(all="ignore"):
                ph = mr.photons_build(*[self.cells[n] for n in RAD_NAMES], np.full((1, 1), self.p), self.B, side)
            self._ph[side] = {key: np.broadcast_to(v, self.shape[1:]) for key, v in ph.items()}
        return self._ph[side]

    def all_sides(self, form, *args):
        """grid / series / band under the three decisions of the spectrum's thresholds (exact, just below, just above): a FluxSides."""
        return FluxSides([getattr(self, form)(*args, side=s) for s in (None, -1, +1)])

    def boundary(self, i, j, k, lg2_nu_obs, side=None):
        """log2 I_nu'(cell (j, k), log2 nu + log2(1+z) - lg2_doppler) + lg2_geom at the lattice nodes (i, j, k) (index arrays that
        broadcast against lg2_nu_obs, log2 of the observed frequency in code units).  A value beyond the double range is -inf, as in
        the double computation this restates (the exponential cut-off far past nu_M)."""
        B = self.B
        i, j, k, x = np.broadcast_arrays(i, j, k, lg2_nu_obs)
        with np.errstate(all="ignore"):
            ph = {key: v[j, k] for key, v in self.photons(side).items()}
            x = x + B.log2(1 + B.const(self.z)) - self.lat["lg2_doppler"][i, j, k]
            geom = self.lat["lg2_geom"][i, j, k]
            if self.geom_shift is not None:
                (si, sj, sk), delta = self.geom_shift
                geom = geom + np.where((i == si) & (j == sj) & (k == sk), B.const(delta), B.const(0.0))
            b = mr.log2_I_nu(ph, x, B, side) + geom
            return np.where(mr.to_float(b) == -np.inf, B.const(-np.inf), b)

    def _sum(self, lg2_t_req, lg2_nu, series, through, keep_terms, side=None):
        """Grid form (series False): [L][n] over times x frequencies; series form: [n] over the (t, nu) pairs."""
        B = self.B
        npe, nth, K = self.shape
        n = lg2_t_req.size
        k, inside, edge = _brackets(self.lat["lg2_t"], self.lat["lg2_t_ulp"], lg2_t_req, through)  # [npe][nth][n]
        ii, jj = np.arange(npe)[:, None, None], np.arange(nth)[None, :, None]
        if series:
            lo, hi = self.boundary(ii, jj, k, lg2_nu[None, None, :], side), self.boundary(ii, jj, k + 1, lg2_nu[None, None, :], side)
            sel = (ii, jj, k)
        else:  # every node's spectrum once per frequency, as specific_flux stages them
            kk = np.arange(K)[None, None, :, None]
            bnd = self.boundary(ii[..., None], jj[..., None], kk, lg2_nu[None, None, None, :], side)  # [npe][nth][K][L]
            lo = np.moveaxis(np.take_along_axis(bnd, k[..., None], axis=2), 3, 2)  # [npe][nth][L][n]
            hi = np.moveaxis(np.take_along_axis(bnd, (k + 1)[..., None], axis=2), 3, 2)
            sel = (ii, jj, k)
        t_lo, t_hi = self.lat["lg2_t"][sel], self.lat["lg2_t"][ii, jj, k + 1]
        dt, dT = t_hi - t_lo, lg2_t_req[None, None, :] - t_lo
        if not series:
            dt, dT, inside, edge = dt[:, :, None, :], dT[:, :, None, :], inside[:, :, None, :], edge[:, :, None, :]
        with np.errstate(all="ignore"):
            slope = (hi - lo) / dt
            ok = np.isfinite(mr.to_float(slope))  # (a slope beyond the double range is not finite in the double computation either)
            col = np.where(ok, lo + dT * np.where(ok, slope, 0 * slope), B.const(-np.inf))
            term = B.exp2(col)
        for (si, sj) in self.skip_rows:
            term[si, sj] = 0 * term[si, sj]
        add = np.where(inside, term, 0 * term)
        total = add.sum(axis=(0, 1))
        alt = {}
        edge_b = np.broadcast_to(edge, term.shape) & np.asarray(term != 0, dtype=bool)
        for idx in zip(*np.nonzero(edge_b)):  # slot -> {row: the signed term the other decision adds}
            q = int(np.ravel_multi_index(idx[2:], total.shape))
            v = term[idx]
            alt.setdefault(q, {})[idx[:2]] = -v if np.broadcast_to(inside, term.shape)[idx] else v
        return total, alt, (add if keep_terms else None)

    def _flux(self, total, alt, terms, unit):
        k = _norm(self.z, self.lumi_dist, self.B) / self.B.const(unit)
        return Flux(total * k, {q: [v * k for v in d.values()] for q, d in alt.items()}, None if terms is None else terms * k)

    def _requests(self, t, nu, lg2_t):
        t_code = np.asarray(t, dtype=np.float64) * mr.U_SEC  # (the double product every producer forms before its log2)
        nu_code = np.asarray(nu, dtype=np.float64) * U_HZ
        return (self.B.log2(self.B.arr(t_code)) if lg2_t is None else lg2_t), self.B.log2(self.B.arr(nu_code))

    def grid(self, t, nu, keep_terms=False, lg2_t=None, side=None):
        """specific_flux: flux density [nnu][nt] in erg cm^-2 s^-1 Hz^-1 at times t [s] and frequencies nu [Hz].  lg2_t (backend
        values, log2 of the time in code units) replaces log2 t: a request no double can make, placed exactly on a lattice node."""
        lt, ln = self._requests(t, nu, lg2_t)
        return self._flux(*self._sum(lt, ln, False, False, keep_terms, side), U_FLUX_DEN_CGS)

    def series(self, t, nu, keep_terms=False, through=True, lg2_t=None, side=None):
        """specific_flux_series: flux density [n] at the (t, nu) pairs (in any order: every point finds its own bracket).
        through=False brackets with iterate_to, as the grid form does; lg2_t as in grid()."""
        lt, ln = self._requests(t, nu, lg2_t)
        return self._flux(*self._sum(lt, ln, True, through, keep_terms, side), U_FLUX_DEN_CGS)

    def band(self, t, nu_min, nu_max, num_nu, side=None):
        """Observer::flux: the Boole sum of the grid form over num_nu log-spaced frequencies [nt], erg cm^-2 s^-1."""
        B = self.B
        nu_code = band_nodes(nu_min, nu_max, num_nu)
        w = boole_weights(nu_code, B)
        lt = B.log2(B.arr(np.asarray(t, dtype=np.float64) * mr.U_SEC))
        total, alt, _ = self._sum(lt, B.log2(B.arr(nu_code)), False, False, False, side)
        n = lt.size
        balt = {}  # a row is in or out at a time for every frequency at once
        for q, d in alt.items():
            for row, v in d.items():
                slot = balt.setdefault(q % n, {})
                slot[row] = slot.get(row, 0) + v * w[q // n]
        return self._flux((total * w[:, None]).sum(axis=0), balt, None, U_FLUX_CGS)


def band_nodes(nu_min, nu_max, num_nu):
    """logspace(log10 nu_min, log10 nu_max, num_nu) in code units, in double as every producer forms its nodes."""
    a, b = np.log10(np.float64(nu_min) * U_HZ), np.log10(np.float64(nu_max) * U_HZ)
    step = (b - a) / max(1.0, float(num_nu - 1))
    e = np.array([b if (num_nu > 1 and i == num_nu - 1) else a + step * i for i in range(num_nu)])
    return np.power(10.0, e)


def boole_weights(grid, B=mr.DEFAULT):
    """compute_boole_weights: composite Boole panels of four intervals in ln nu, the rest by Simpson 3/8, Simpson or trapezoid."""
    g = B.arr(grid)
    n = g.size
    w = np.zeros(n, dtype=g.dtype) + B.const(0.0)
    if n < 2:
        return w
    h = (B.log2(g[1:2]) - B.log2(g[0:1]))[0] / B.log2e()
    cb = 2 * h / 45
    j = 0
    while j + 4 < n:
        for o, c in enumerate((7, 32, 12, 32, 7)):
            w[j + o] += cb * c
        j += 4
    rest = n - 1 - j
    tail = {3: [(3 * h / 8) * c for c in (1, 3, 3, 1)], 2: [(h / 3) * c for c in (1, 4, 1)], 1: [h / 2, h / 2]}.get(rest, [])
    for o, c in enumerate(tail):
        w[j + o] += c
    return w * g
