"""Extended-precision reference of the forward-shock blast wave of one (model, theta) row without lateral spreading, energy injection
or a reverse shock: the SOLUTION of the equations at given times, for tests/test_dyn_solution_host.py (the CPU checker) and
tests/test_dyn_solution.py (the three device kernels).  numpy.longdouble (64-bit mantissa on x86-64).

The problem, from the physics as the kernel headers cite it (not from FsRhs' rewritten algebra):
  * ForwardShockEqn::operator() (forward-shock.tpp:10-70) in its textbook form -- gamma_c = (gamma_bar + sqrt(gamma_bar^2 + 4)) / 2,
    eps_rad = eps_e (gamma_m / gamma_c)^(p-2) in slow cooling and eps_e in fast cooling (0 without radiative_fireball),
    ad = 4/3 + 1/(3 Gamma), Gamma_eff = (ad (Gamma^2 - 1) + 1) / Gamma, and the derivatives of Gamma, m2, U, r, t_comv;
  * the media: ISM and the analytic wind rho = A / (r02 + r^2) + rho_ism;
  * set_init_state (forward-shock.tpp:120-149): t0 = min(t_first, 0.1 s, 0.1 t_dec), r0, t_comv0, m2 = enclosed mass, U = enclosed
    thermal energy (closed form in the ISM, the 32-panel Simpson rule in ln r otherwise: both are part of the problem's statement);
  * t_dec, which enters t0 only: the estimate of grid-refinement.h:402-453, restated in float64;
  * fwd_shock_state: Gamma_th = U / (m2 c^2) + 1, B = sqrt(8 pi eps_B e_th) with the compression ratio (ad Gamma + 1) / (ad - 1),
    N_p = m2 / m_p.

The integrator is NOT DOPRI5: Gragg's modified midpoint rule in ln t, extrapolated (Aitken-Neville on the step numbers 2, 4, ..., 2 K_ORDER:
order 2 K_ORDER), with fixed steps of at most H_MAX in ln t that end on the requested times -- no interpolation.  The one place where the
right-hand side is not smooth, gamma_m = gamma_c (the power of eps_rad switches on or off there: a kink), is located (secant on
ln(gamma_m / gamma_c) over the step's length) and stepped onto: each side of it is integrated with its own smooth branch.  Rows are
vectorised: every row carries its own list of steps.

Energy.  With eps_rad = 0 the equations give d/dt [Gamma (m_jet0 + m2) + Gamma_eff U - m2] = U (dGamma_eff/d ad) (d ad/d Gamma) dGamma/dt:
the dGamma/dt equation carries dGamma_eff/dGamma at constant ad (forward-shock.tpp: dGamma_eff = (ad (Gamma^2 + 1) - 1) / Gamma^2), so the
sum E is conserved only up to the integral W of that right-hand side, -U (Gamma^2 - 1) / (3 Gamma^3) dGamma.  The reference carries W as
a sixth variable; E - W is the invariant it has to hold (test_dyn_solution_host.py), and E_ref(t) = E(t0) + W(t) is what a solver's E is
held to."""
import math

import numpy as np

LD = np.longdouble

# units and constants: the float64 expressions of vag_device.h / oracle/vag_oracle.c (they define the problem's parameters)
U_LEN = 1.5e13
U_CM = 1 / U_LEN
U_SEC = 3e10 / U_LEN
U_CM3 = U_CM * U_CM * U_CM
U_G = 1 / 2e33
U_GAUSS = 8.66e-11 / U_SEC
U_ERG = U_G * U_CM * U_CM / U_SEC / U_SEC
C_C = 1.0
C_MP = 1.67e-24 * U_G
C_ME = C_MP / 1836
C_SIGMAT = 6.65e-25 * U_CM * U_CM
GAMMA_CUT = 1.0 + 1e-6
FLAG_SPREADING, FLAG_MAGNETAR, FLAG_RVS = 32, 64, 4

H_MAX = 0.25   # longest step in ln t
K_ORDER = 6    # extrapolation columns: order 12
SLOW, FAST = 0, 1
EVENT_TOL = LD(1e-10)  # |ln(gamma_m / gamma_c)| at a located kink; an error d there costs ~0.03 d^2 in the state

QUANTITIES = ("Gamma", "Gamma-1", "r", "t_comv", "m2", "Gamma_th-1", "B")

# ---- the models of the tests: the smallest shapes at which the solver can still go wrong ----
T_WIN = (1e2, 1e8)
LOW = (0.01, 0.01, 2.0)  # (phi, theta, t) resolutions: 36 to 38 theta rows (the grid's minimum), 17 to 21 nodes per row
_A = dict(jet="TophatJet", theta_c=0.1, E_iso=1e52, Gamma0=300.0, medium="ISM", n_ism=1.0, lumi_dist=1e28, z=1.0, theta_obs=0.0,
          eps_e=0.1, eps_B=0.01, p=2.3, resolutions=LOW)
_C4 = dict(jet="GaussianJet", theta_c=0.07, E_iso=10 ** 52.4, Gamma0=500.0, medium="ISM", n_ism=1e-2, lumi_dist=1.23e26, z=0.0098,
           theta_obs=0.4, eps_e=10 ** -1.5, eps_B=10 ** -3.5, p=2.15)  # configs.C4_TRUTH
_PLW = dict(_A, jet="PowerLawJet", medium="Wind", k_e=2.0, k_g=2.0, A_star=0.1, n_ism=0.0, theta_obs=0.2)
MODELS = {
    "a_tophat_ism": _A,
    "b_c4_gaussian": dict(_C4, resolutions=LOW),
    "c_powerlaw_wind": _PLW,
    "c_powerlaw_wind_floor": dict(_PLW, n_ism=1e-3),
    # d: eps_rad = eps_e for every p <= 2, so the two have one solution; they are here for the branch (pm2 = 0, gm_coeff < 0 and = 0)
    "d_p_1.9": dict(_A, p=1.9),
    "d_p_2": dict(_A, p=2.0),
    "e_adiabatic": dict(_A, radiative_fireball=False),
    "e_adiabatic_gaussian_wind": dict(_C4, medium="Wind", A_star=0.1, n_ism=0.0, radiative_fireball=False, resolutions=LOW),
    "f_fast_cooling": dict(_A, eps_e=0.5, eps_B=0.1, n_ism=1e3),
    "g_gamma0_1.5": dict(_A, Gamma0=1.5, resolutions=(0.01, 0.01, 3.0)),  # (its lattice starts late: 12 nodes at 2 per decade)
    "g_gamma0_2000": dict(_A, Gamma0=2000.0),
    # h: model a is itself the lowest time resolution that leaves 16 nodes (17; steps that pass no node); this is the dense end
    "h_time_high": dict(_A, resolutions=(0.01, 0.01, 100.0)),
    "i_c4_gaussian_65_rows": dict(_C4, resolutions=(0.01, 1.3, 2.0)),
    "i_powerlaw_wind_65_rows": dict(_PLW, resolutions=(0.01, 0.35, 2.0)),
}
ADIABATIC = ("e_adiabatic", "e_adiabatic_gaussian_wind")
REFILL = ("i_c4_gaussian_65_rows", "i_powerlaw_wind_65_rows")
SWEEP = {"a_tophat_ism": _A, "sweep_gaussian_wind": dict(_C4, medium="Wind", A_star=0.1, n_ism=0.0, resolutions=LOW)}
SWEEP_RTOL = (1e-4, 1e-6, 1e-8)


def select_rows(theta, theta_c, theta_obs):
    """First, last, nearest theta_c, nearest the line of sight, then every ceil(n / 8)-th row: at most 12."""
    n = len(theta)
    rows = {0, n - 1, int(np.argmin(np.abs(theta - theta_c))), int(np.argmin(np.abs(theta - theta_obs)))}
    rows.update(range(0, n, -(-n // 8)))
    return sorted(rows)


def round_up(x):
    """x rounded up to two digits."""
    if not 0 < x < math.inf:
        return x if x == math.inf else 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f"{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.1e}")


def checker_side(oracle, name, kw=None, rtol=1e-6):
    """(details, selected rows, reference job) of one model through the checker."""
    import _abi
    kw = dict(MODELS[name] if kw is None else kw, rtol=rtol)
    prm = _abi.make_params(**kw)
    d = oracle.details(prm, *T_WIN)
    rows = select_rows(d["theta"], kw["theta_c"], kw["theta_obs"])
    job = (prm, oracle.profile(prm, 0, d["theta"][rows]), oracle.profile(prm, 1, d["theta"][rows]), d["t_src"][rows])
    return d, rows, job


# ---- the problem's statement ----
def _medium(prm):
    rho_ism = (prm.n_ism / U_CM3) * C_MP
    if prm.medium_type == 0:
        return rho_ism, 0.0, 0.0
    assert prm.k_m == 2, "the analytic wind only"
    A = prm.A_star * 5e11 * U_G / U_CM
    return rho_ism, A, A / ((prm.n0 / U_CM3) * 1.3 * C_MP)


def _rho(P, r):
    return P["A"] / (P["r02"] + r * r) + P["rho_ism"]


def _mass(P, r):  # enclosed_mass_medium, shock-physics.h:439-446
    a = np.sqrt(P["r02"])
    with np.errstate(all="ignore"):
        wind = np.where(a > 0, r - a * np.arctan(r / np.where(a > 0, a, 1)), r)
    return P["rho_ism"] * r ** 3 / 3 + P["A"] * wind


def _thermal_energy(P, r, G, eps_e):  # enclosed_thermal_energy_medium, shock-physics.h:401-468
    ad = LD(4) / 3 + 1 / (3 * G)
    cool = 3 * (ad - 1)
    ism = P["rho_ism"] * r ** 3 * (1 - np.exp(LD(-18) * (3 + cool))) / (3 + cool)
    n = 32
    u_max = np.log(r)
    h = LD(18) / n
    total = 0
    for i in range(n + 1):
        ri = np.exp(u_max - 18 + i * h)
        total = total + (1 if i in (0, n) else 4 if i % 2 else 2) * _rho(P, ri) * ri ** 3 * (ri / r) ** cool
    return (1 - eps_e) * (G - 1) * C_C ** 2 * np.where(P["wind"], total * h / 3, ism)


def t_dec_estimate(eps_k, G0, rho_ism, A, r02, wind):
    """estimate_t_dec (grid-refinement.h:402-453) of one row, float64: it enters t0 only."""
    beta = math.sqrt((G0 - 1) * (G0 + 1)) / G0
    target = eps_k / (G0 * C_C ** 2) / G0
    kin = (1 - beta) / (beta * C_C)
    r_min = 1e-3
    if target <= 0:
        return r_min * kin
    if not wind:
        return min(np.cbrt(max(r_min ** 3 + 3 * target / rho_ism, 0.0)), r_min * 1e40) * kin if rho_ism > 0 else r_min * 1e40 * kin
    n = 256
    u_min = math.log(1e-3)
    du = 40 * math.log(10.0) / n
    dens = lambda r: A / (r02 + r * r) + rho_ism
    mass, r_prev = 0.0, math.exp(u_min)
    f_prev = dens(r_prev) * r_prev * r_prev
    for i in range(1, n + 1):
        r_i = math.exp(u_min + i * du)
        f_i = dens(r_i) * r_i * r_i
        panel = 0.5 * (f_prev + f_i) * (r_i - r_prev)
        if mass + panel >= target:
            return (r_prev + (target - mass) / f_i) * kin
        mass, f_prev, r_prev = mass + panel, f_i, r_i
    return math.exp(u_min + 40 * math.log(10.0)) * kin


def _rows(prm, E_iso, Gamma0, t_src):
    """The per-row parameters (longdouble arrays) and start of the rows of one model; t_src [s] is (rows, nodes)."""
    assert not prm.flags & (FLAG_SPREADING | FLAG_MAGNETAR | FLAG_RVS) and prm.jet_type in (0, 1, 2), "outside the reference's scope"
    n = len(E_iso)
    rho_ism, A, r02 = _medium(prm)
    full = lambda v: np.full(n, v, dtype=LD)
    G0 = np.asarray(Gamma0, dtype=LD)
    eps_k = np.asarray(E_iso, dtype=np.float64) * U_ERG / (4 * math.pi)
    P = dict(rho_ism=full(rho_ism), A=full(A), r02=full(r02), wind=np.full(n, prm.medium_type != 0),
             m_jet0=eps_k.astype(LD) / G0 / C_C ** 2,
             gm_coeff=full((prm.p - 2) / (prm.p - 1) * prm.eps_e * C_MP / C_ME / prm.xi_e),
             gc_coeff=full(6 * math.pi * C_ME * C_C / C_SIGMAT / (8 * math.pi * prm.eps_B)),
             eps_e=full(prm.eps_e if prm.radiative_fireball else 0.0), pm2=full(prm.p - 2),
             kink=np.full(n, bool(prm.radiative_fireball) and prm.p > 2), eps_B=full(prm.eps_B))
    nodes = np.asarray(t_src, dtype=LD) * U_SEC
    t_dec = np.array([t_dec_estimate(float(eps_k[j]), float(Gamma0[j]), rho_ism, A, r02, prm.medium_type != 0) if Gamma0[j] > 1 else 1.0
                      for j in range(n)])
    t0 = np.minimum(nodes[:, 0], LD(min(0.1 * U_SEC, 1e300))).astype(LD)
    t0 = np.minimum(t0, (0.1 * t_dec).astype(LD))
    with np.errstate(all="ignore"):  # rows at Gamma0 = 1 (stopped) give 0 / 0 in t_comv0
        u0 = np.sqrt((G0 - 1) * (G0 + 1))
        beta = u0 / G0
        r0 = beta * C_C * t0 * G0 * G0 * (1 + beta)
        tc0 = r0 / u0 / C_C
        y0 = np.array([G0 - 1, _mass(P, r0), _thermal_energy(P, r0, G0, P["eps_e"]), r0, tc0, np.zeros(n, dtype=LD)])
    return P, y0, t0, nodes, G0


def _take(P, idx):
    return {k: v[idx] for k, v in P.items()}


def _ln_ratio(P, y, t):
    """ln(gamma_m / gamma_c) (RadiativeEfficiency, shock-physics.h:247-288); 0 where the row has no kink."""
    g, r, tc = y[0], y[3], y[4]
    with np.errstate(all="ignore"):
        e_th = g * 4 * (1 + g) * _rho(P, r) * C_C ** 2
        gamma_bar = P["gc_coeff"] / (e_th * tc)
        gamma_c = (gamma_bar + np.sqrt(gamma_bar * gamma_bar + 4)) / 2
        gamma_m = P["gm_coeff"] * g + 1
        return np.where(P["kink"], np.log(gamma_m / gamma_c), 0)


def _f(P, y, t, mode):
    """d/d(ln t) of (Gamma - 1, m2, U, r, t_comv, W): t times ForwardShockEqn::operator().  The state carries g = Gamma - 1, so that a
    row that starts or ends at Gamma - 1 ~ 1e-9 keeps its digits; Gamma^2 - 1 = g (g + 2)."""
    g, m2, U, r = y[0], y[1], y[2], y[3]
    G = 1 + g
    u = np.sqrt(g * (g + 2))
    dr = u * (G + u) * C_C        # beta c / (1 - beta), written without the cancellation (compute_dr_dt)
    dtc = G + u                   # 1 / (Gamma (1 - beta))
    dm = r * r * _rho(P, r) * dr
    eps_rad = P["eps_e"]
    if P["kink"].any():
        eps_rad = eps_rad * np.where(P["kink"] & (mode == SLOW), np.exp(P["pm2"] * _ln_ratio(P, y, t)), 1)
    ad = LD(4) / 3 + 1 / (3 * G)
    G_eff = (ad * g * (g + 2) + 1) / G
    dG_eff = (ad * (G * G + 1) - 1) / (G * G)
    dlnV = 3 / r * dr
    a1 = -g * (G_eff + 1) * C_C ** 2 * dm
    a2 = (ad - 1) * G_eff * U * dlnV
    b1 = (P["m_jet0"] + m2) * C_C ** 2
    b2 = (dG_eff + G_eff * (ad - 1) / G) * U
    dG = (a1 + a2) / (b1 + b2)
    dU = (1 - eps_rad) * g * C_C ** 2 * dm - (ad - 1) * (dlnV - dG / G) * U
    dW = -U * g * (g + 2) / (3 * G ** 3) * dG  # U (dGamma_eff / d ad) (d ad / dGamma) dGamma
    return t * np.array([dG, dm, dU, dr, dtc, dW])


def _gbs(P, y, s, H, mode, K):
    """One extrapolated modified-midpoint step of length H (per row) in s = ln t."""
    f0 = _f(P, y, np.exp(s), mode)
    T = []
    for j in range(K):
        n = 2 * (j + 1)
        h = H / n
        z0, z1 = y, y + h * f0
        for m in range(1, n):
            z0, z1 = z1, z0 + 2 * h * _f(P, z1, np.exp(s + m * h), mode)
        row = [(z0 + z1 + h * _f(P, z1, np.exp(s + H), mode)) / 2]
        for k in range(1, j + 1):
            ratio = LD(n) / (2 * (j - k + 1))
            row.append(row[k - 1] + (row[k - 1] - T[j - 1][k - 1]) / (ratio * ratio - 1))
        T.append(row)
    return T[-1][-1]


def _advance(P, y, s, H, mode, K, depth=0):
    """A step of every row, split at the kink where a row crosses it; returns the new state and cooling branch."""
    y1 = _gbs(P, y, s, H, mode, K)
    if not P["kink"].any():
        return y1, mode
    g1 = _ln_ratio(P, y1, np.exp(s + H))
    bad = P["kink"] & (H > 0) & (((mode == SLOW) & (g1 > EVENT_TOL)) | ((mode == FAST) & (g1 < -EVENT_TOL)))
    if not bad.any():
        return y1, mode
    assert depth < 4, "the cooling branch changes more than four times inside one step"
    idx = np.nonzero(bad)[0]
    Q, ya, sa, Ha, ma = _take(P, idx), y[:, idx], s[idx], H[idx], mode[idx]
    # Illinois iteration on g(x) = ln ratio after a step of length x from the step's start, in the branch of the start
    a, fa = np.zeros(len(idx), dtype=LD), _ln_ratio(Q, ya, np.exp(sa))
    b, fb = Ha.copy(), g1[idx]
    immediate = fa * fb > 0  # the start already sits on the kink (a crossing just located): change branch at once
    x, yx = b.copy(), y1[:, idx]
    for _ in range(60):
        with np.errstate(all="ignore"):
            x = np.where(immediate, 0, np.where(fb != fa, b - fb * (b - a) / (fb - fa), (a + b) / 2))
        yx = _gbs(Q, ya, sa, x, ma, K)
        fx = np.where(immediate, 0, _ln_ratio(Q, yx, np.exp(sa + x)))
        if np.all(np.abs(fx) <= EVENT_TOL):
            break
        same = fx * fb > 0
        a, fa = np.where(same, a, b), np.where(same, fa / 2, fb)
        b, fb = x, fx
    else:
        raise AssertionError("the kink gamma_m = gamma_c was not located")
    y_rest, m_rest = _advance(Q, yx, sa + x, Ha - x, 1 - ma, K, depth + 1)
    y1, mode = y1.copy(), mode.copy()
    y1[:, idx], mode[idx] = y_rest, m_rest
    return y1, mode


def solve(P, y0, t0, nodes, refine=1, h_max=H_MAX, K=K_ORDER):
    """The state (6, rows, nodes) at the nodes: steps of at most h_max / refine in ln t from t0, ending on every node."""
    n, nt = nodes.shape
    s_nodes = np.log(nodes)
    prev = np.log(t0)
    starts, lengths, marks = [], [], []  # per row: step starts, step lengths, node index the step ends on (or -1)
    gaps = np.diff(np.concatenate([prev[:, None], s_nodes], axis=1), axis=1)
    assert np.all(gaps >= 0), "node times must ascend from t0"
    subs = np.maximum(1, np.ceil(gaps.astype(np.float64) / h_max).astype(int)) * refine
    L = int(subs.sum(axis=1).max())
    S, Hs, M = np.zeros((n, L), dtype=LD), np.zeros((n, L), dtype=LD), np.full((n, L), -1)
    for j in range(n):
        i = 0
        for k in range(nt):
            base = prev[j] if k == 0 else s_nodes[j, k - 1]
            h = gaps[j, k] / subs[j, k]
            for q in range(subs[j, k]):
                S[j, i], Hs[j, i] = base + q * h, (h if q + 1 < subs[j, k] else s_nodes[j, k] - (base + q * h))
                i += 1
            M[j, i - 1] = k
        S[j, i:] = s_nodes[j, -1]  # rows with fewer steps idle at their last node (steps of length zero)
    y = y0.copy()
    mode = np.where(_ln_ratio(P, y, t0) < 0, SLOW, FAST)
    out = np.zeros((6, n, nt), dtype=LD)
    for i in range(L):
        y, mode = _advance(P, y, S[:, i], Hs[:, i], mode, K)
        hit = np.nonzero(M[:, i] >= 0)[0]
        out[:, hit, M[hit, i]] = y[:, hit]
    return out


def energy(m_jet0, g, m2, U):
    """Gamma (m_jet0 + m2) + Gamma_eff U - m2 from g = Gamma - 1, masses in energy units."""
    G = 1 + g
    ad = LD(4) / 3 + 1 / (3 * G)
    return (G * m_jet0 + g * m2) * C_C ** 2 + (ad * g * (g + 2) + 1) / G * U


def compression(G):
    """Shock compression ratio for an upstream at rest: (ad Gamma + 1) / (ad - 1)."""
    ad = LD(4) / 3 + 1 / (3 * G)
    return (ad * G + 1) / (ad - 1)


def compression_4vel(G):
    """The same from the jump conditions' four-velocities (shock.cpp:93-100, shock-physics.h:190-203), as the code forms it."""
    ad = LD(4) / 3 + 1 / (3 * G)
    u_down = np.sqrt((G - 1) * (ad - 1) ** 2 / (-ad * (ad - 2) * (G - 1) + 2))
    return (np.sqrt((1 + u_down * u_down) * (G - 1) * (G + 1)) + u_down * G) / u_down


def reference(jobs, refine=1, h_max=H_MAX, K=K_ORDER):
    """jobs: a list of (params, E_iso[rows], Gamma0[rows], t_src[rows][nodes] in seconds).  Returns per job a dict of (rows, nodes)
    longdouble arrays in the units of Model.details (Gamma, Gamma-1, r [cm], t_comv [s], m2 [code], Gamma_th-1, B [G]) plus U, W, E (the
    energy sum), E0, m_jet0 and `stopped` (rows at or below GAMMA_CUT: their r, t_comv are set_stopping_shock's constants).  Identical
    rows are solved once, and all jobs with the same node count in one vectorised pass."""
    made = [_rows(*job) for job in jobs]
    results = [None] * len(jobs)
    for nt in sorted({m[3].shape[1] for m in made}):
        group = [i for i, m in enumerate(made) if m[3].shape[1] == nt]
        P = {k: np.concatenate([made[i][0][k] for i in group]) for k in made[group[0]][0]}
        y0 = np.concatenate([made[i][1] for i in group], axis=1)
        t0 = np.concatenate([made[i][2] for i in group])
        nodes = np.concatenate([made[i][3] for i in group])
        G0_all = np.concatenate([made[i][4] for i in group])
        live = np.nonzero(G0_all > GAMMA_CUT)[0]
        keys = {}
        for j in live:
            key = tuple(v[j].tobytes() for v in P.values()) + (y0[:, j].tobytes(), nodes[j].tobytes())
            keys.setdefault(key, []).append(j)
        first = np.array([v[0] for v in keys.values()], dtype=int)
        sol = np.zeros((6, len(t0), nt), dtype=LD)
        if len(first):
            part = solve(_take(P, first), y0[:, first], t0[first], nodes[first], refine, h_max, K)
            for q, rows in enumerate(keys.values()):
                sol[:, rows, :] = part[:, q:q + 1, :]
        at = 0
        for i in group:
            n = len(made[i][2])
            sl = slice(at, at + n)
            at += n
            g, m2, U, r, tc, W = sol[:, sl, :]
            G = 1 + g
            stopped = G0_all[sl] <= GAMMA_CUT
            Pj = _take(P, sl)
            with np.errstate(all="ignore"):
                gth1 = U / (m2 * C_C ** 2)
                B = np.sqrt(8 * LD(math.pi) * Pj["eps_B"][:, None] * gth1 * _rho({k: v[:, None] for k, v in Pj.items()}, r) * compression(G) * C_C ** 2)
            res = dict(stopped=stopped, U=U, W=W, m_jet0=Pj["m_jet0"], E=energy(Pj["m_jet0"][:, None], g, m2, U),
                       E0=energy(Pj["m_jet0"], *y0[:3, sl]), t0=t0[sl])
            res.update({"Gamma": G, "Gamma-1": g, "r": r / U_CM, "t_comv": tc / U_SEC, "m2": m2, "Gamma_th-1": gth1, "B": B / U_GAUSS})
            for name, v0 in (("r", y0[3, sl] / U_CM), ("t_comv", y0[4, sl] / U_SEC)):
                res[name] = np.where(stopped[:, None], v0[:, None], res[name])
            results[i] = res
    return results


def side_values(d, rows):
    """The compared quantities of a details dict (the checker's or the device's) on the selected rows, in longdouble."""
    g = lambda n: np.asarray(d[n])[rows].astype(LD)
    m2 = g("N_p") * C_MP
    return {"Gamma": g("Gamma"), "Gamma-1": g("Gamma") - 1, "r": g("r"), "t_comv": g("t_comv"), "m2": m2,
            "Gamma_th-1": g("Gamma_th") - 1, "B": g("B"), "U": (g("Gamma_th") - 1) * m2 * C_C ** 2}


def errors(d, rows, ref, keep=None):
    """Maximum relative error per quantity over every node of the rows that are not stopped (and, where `keep` is given, kept), and the
    list of what is wrong with the stopped ones.  Gamma_th - 1 is charged only what exceeds the rounding of the stored Gamma_th,
    2^-52 / (Gamma_th - 1).  (No grid of tests' models holds a stopped row -- the theta range ends where Gamma0 reaches GAMMA_CUT from
    above, test_dyn_solution_host.py asserts it -- so the stopped branch below waits for a model that has one.)"""
    v = side_values(d, rows)
    live = ~ref["stopped"] if keep is None else ~ref["stopped"] & np.asarray(keep)
    worst, problems = {}, []
    for q in QUANTITIES:
        with np.errstate(all="ignore"):
            e = np.abs(v[q][live] - ref[q][live]) / np.abs(ref[q][live])
            if q == "Gamma_th-1":
                e = np.maximum(e - LD(2.0 ** -52) / ref[q][live], 0)
        if e.size:
            worst[q] = float(np.max(e)) if np.all(np.isfinite(e)) else float("inf")
    s = ref["stopped"]
    if s.any():  # set_stopping_shock (shock-physics.h:388-397)
        for name, want in (("Gamma", 1), ("Gamma_th", 1), ("B", 0), ("N_p", 0)):
            if not np.all(np.asarray(d[name])[rows][s] == want):
                problems.append(f"stopped row: {name} is not {want}")
        for name in ("r", "t_comv"):
            got = np.asarray(d[name])[rows][s].astype(LD)
            if not np.all(np.abs(got - ref[name][s]) <= 1e-14 * np.abs(ref[name][s])):
                problems.append(f"stopped row: {name} is not its start value")
    return worst, problems


def energy_drift(d, rows, ref):
    """Per selected row: max over the nodes of |E_side - (E(t0) + W)| / E(t0), E formed in longdouble from the side's Gamma, m2, U."""
    v = side_values(d, rows)
    E = energy(ref["m_jet0"][:, None], v["Gamma-1"], v["m2"], v["U"])
    with np.errstate(all="ignore"):
        drift = np.max(np.abs(E - (ref["E0"][:, None] + ref["W"])) / ref["E0"][:, None], axis=1)
    return np.where(ref["stopped"], 0, drift).astype(np.float64)
