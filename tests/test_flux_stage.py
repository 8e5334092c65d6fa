"""The device's synchrotron flux stage -- the equal-arrival-time lattice of every (theta, phi) row, the two boundary spectra of a time's
bracket, the log-log interpolation, exp2 and the row sum -- against the extended-precision reference of that stage alone
(tests/_fluxref.py), fed with the device's OWN intermediates: Model.details of the same model and window gives phi, theta, t_src, r,
Gamma, the polar angle per cell and the five radiation arrays; the reference lays out the lattice itself and sums in long double.  Both
calls lay their grid out with vag_grid_kernel on the same (t_min, t_max) (details_impl and the flux entry points of vag_capi.hip both
run run_model_stages on the extrema of the requested times), so nothing of the ODE, the grids or the electrons enters the comparison.

Every kernel form of the stage is selected by the library's hooks and confirmed from its VAG_DEBUG_LAUNCH report.  Requested times are
taken from the device's own lattice (Model.details' t_obs): on and next to interior and first nodes of three rows.  In these models no
row's LAST node lies inside a window one can request -- the grid ends 1 % past t_max (asserted in `standard_request`) -- so that sub-case
is dropped.  Series times must ascend (the API's contract), so a "shuffled" series shuffles the frequencies of repeated times.

Not covered: SSC components (their tables are not in the details), non-axisymmetric jets, exposure averaging.

What the first measurement found (MI355X, 2026-10-17): every form of the stage within 4e-12 of the reference, so no defect of the flux
kernels; and vag_eat_details_kernel, the side check, at 8.1e-12 (t_obs) / 3.1e-11 (Doppler) on the on-axis top hat against its ceiling of
1e-13 -- it formed 1 - cos_v and Gamma - u cos_v with their cancellations.  That kernel was rewritten (vag_kernels.h); the constants
below are those of the rewritten kernel.

Metric: relative error per slot, the bound scaled by max(1, |log2 reference| / 256) where the slot sits in the exponential cut-off; a slot
whose reference is exactly 0 must be 0, one below 1e-250 must be below 1e-250, and at most 2 % of a request's slots may be such.  Every
slot is compared with the nearest of the reference's admissible values: the two bracket decisions at a row's first node, and the three
decisions of the spectrum's own thresholds (_fluxref.FluxSides)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _abi
import _fluxref as fr
import _mathref as mr
import configs
import vegasafterglow_amd as va
from test_flux_persistent import jittered
from vegasafterglow_amd import _lib
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

GATE_FACTOR = 4  # the suite's convention (DEVIANCE_GATE, tests/test_counts.py)
CEILING = 1e-10  # spec_gate (1e-12 in log2) + the roundings of lg2_geom, lg2_doppler at ~250 + a sum of <= 1e5 terms is ~1e-12
EAT_CEILING = 1e-13
# MEASURED[form][model]: the maximum of the metric over the requests of that form and model, measured on an MI355X on 2026-10-17 (rounded
# up to two digits).  The models with head-on, fast cells (the on-axis top hat, the spreading jet, the reverse shock's thick shell) sit
# at 2e-12 ... 4e-12, the others at 1e-14 ... 4e-13: the kernels form the Doppler factor as Gamma - u cos_v in double, which a cell of
# Lorentz factor 300 seen head-on holds to 2 Gamma^2 eps ~ 2e-11 (the CPU oracle shows the same figures against this reference,
# tests/test_flux_stage_host.py).  Every form of one model lands on the same figure to the digits shown: they differ in the order of
# the sum only.  A pair that is missing has not been measured: its test fails after printing its figure.
_WORKGROUP_KERNEL = {"gauss_offaxis": 2.4e-13, "gauss_spread": 2.8e-12, "powerlaw_wind": 2.7e-13, "rs_thick/fwd": 4.0e-13, "rs_thick/rvs": 3.5e-12,
                     "tophat_onaxis": 2.0e-12}
MEASURED = {
    "grid 256 one-item": _WORKGROUP_KERNEL, "grid 256 persistent": _WORKGROUP_KERNEL, "grid 512 one-item": _WORKGROUP_KERNEL,
    "grid 512 persistent": _WORKGROUP_KERNEL, "grid pieces of 8": _WORKGROUP_KERNEL,
    "grid 1x1": {"gauss_offaxis": 2.2e-15},
    "grid 128x4": {"gauss_offaxis": 2.7e-13},
    "grid 171x3": {"gauss_offaxis": 1.5e-14},
    "series per-point": {"gauss_offaxis": 1.5e-14, "tophat_onaxis": 2.1e-12},
    "series fit-rows": {"gauss_offaxis": 1.5e-14, "tophat_onaxis": 2.0e-12, "gauss_offaxis/cut-off": 9.3e-15, "gauss_spread": 2.5e-12},
    "series shared-node": {"gauss_offaxis": 1.5e-14, "tophat_onaxis": 2.0e-12, "gauss_spread": 2.5e-12},
    "grid by series kernel": {"gauss_offaxis": 2.4e-13},
    "grid rows (row per lane)": {"gauss_offaxis batch": 2.2e-13},
    "grid rows counterpart": {"gauss_offaxis batch": 3.7e-13},
    "band of 5": {"gauss_offaxis": 1.3e-14, "gauss_spread": 2.2e-12},
    "band of 9": {"gauss_offaxis": 1.3e-14, "gauss_spread": 2.2e-12},
    "loglike fit-rows": {"gauss_offaxis": 5.1e-15},
}
# model -> (t_obs, Doppler): maximum relative difference of vag_eat_details_kernel from the reference lattice, same machine and date
MEASURED_EAT = {"gauss_offaxis": (6.7e-16, 6.1e-16), "gauss_spread": (1.3e-15, 1.5e-15), "powerlaw_wind": (6.8e-16, 6.6e-16),
                "rs_thick": (5.8e-16, 5.4e-16), "tophat_onaxis": (4.5e-15, 1.9e-14)}

T_LO, T_HI = 1e2, 1e7
NU4 = np.array([1e3, 1e9, 4.84e14, 1e25])  # far below nu_a ... past nu_M + 4 octaves (the exponential cut-off)
SMALL = (0.2, 0.7, 12.0)
MODELS = {
    "tophat_onaxis": dict(configs.C1A, resolutions=SMALL),
    "gauss_offaxis": dict(configs.C4_TRUTH),
    "powerlaw_wind": dict(configs.EXTRA["powerlaw_wind"][0], resolutions=(0.06, 0.2, 5.0)),
    "gauss_spread": dict(jet="GaussianJet", spreading=True, theta_obs=0.15, resolutions=(0.1, 0.3, 5.0)),
    "rs_thick": dict(configs.RS_CASES["rs_thick_offaxis"][0], resolutions=(0.06, 0.3, 8.0)),
}
NU_OF = {"rs_thick": np.array([1e3, 1e9, 4.84e14, 1e22])}  # (the reverse shock's cut-off lies lower: at 1e25 Hz 9 % of its slots are 0)
TABLE = []


@pytest.fixture(scope="module")
def eng():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    h, lock = va.get_context(0)
    yield lib, h
    print("\n[flux stage] form                       model            measured   gate")
    for form, name, err, gate in TABLE:
        print(f"[flux stage] {form:26s} {name:16s} {err:.2e}   {gate if gate is None else format(gate, '.2e')}")


@contextlib.contextmanager
def hooked(capfd, **hooks):
    """The library's hooks for one call, with the launch report on; yields a function that returns the report so far."""
    hooks["VAG_DEBUG_LAUNCH"] = "1"
    for k, v in hooks.items():
        _lib.hooks[k] = v
    capfd.readouterr()
    try:
        yield lambda: capfd.readouterr().err
    finally:
        for k in hooks:
            _lib.hooks.pop(k, None)


def _arr(prms):
    return (_lib.ModelParams * len(prms))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in prms])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dev_grid(eng, prms, t, nu):
    lib, h = eng
    t, nu = _f64(t), _f64(nu)
    out = np.empty((len(prms), nu.size, t.size))
    _lib.check(lib.vag_flux_density_grid_batch(h, _arr(prms), len(prms), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                               out.ctypes.data_as(dp)))
    return out


def dev_grid4(eng, prm, t, nu):
    """(fwd.sync, rvs.sync) of one model's grid."""
    lib, h = eng
    t, nu = _f64(t), _f64(nu)
    comps = [np.empty((nu.size, t.size)) for _ in range(4)]
    arr = (dp * 4)(*[c.ctypes.data_as(dp) for c in comps])
    _lib.check(lib.vag_flux_density_grid_components4_batch(h, _arr([prm]), 1, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                           arr))
    return comps[0], comps[2]


def dev_series(eng, prms, t, nu):
    lib, h = eng
    t, nu = _f64(t), _f64(nu)
    out = np.empty((len(prms), t.size))
    _lib.check(lib.vag_flux_density_batch(h, _arr(prms), len(prms), t.ctypes.data_as(dp), nu.ctypes.data_as(dp), t.size,
                                          out.ctypes.data_as(dp)))
    return out


def dev_band(eng, prms, t, nu_min, nu_max, num_nu):
    lib, h = eng
    t = _f64(t)
    out = np.empty((len(prms), t.size))
    _lib.check(lib.vag_flux_batch(h, _arr(prms), len(prms), t.ctypes.data_as(dp), t.size, float(nu_min), float(nu_max), int(num_nu),
                                  out.ctypes.data_as(dp)))
    return out


# ---- the reference of a model on a window, from the device's details ----
_STAGES = {}


def stages(prm, t_lo, t_hi, key=None):
    """(forward details, [FluxStage of every synchrotron component]) of the model on the window; cached per (key, window)."""
    ck = (key, float(t_lo), float(t_hi))
    if key is not None and ck in _STAGES:
        return _STAGES[ck]
    m = va.Model.from_params(prm)
    d = m.details(float(t_lo), float(t_hi))
    spreading = bool(prm.flags & _lib.FLAG_SPREADING)
    sh = d["shape"]
    n_phi_eff = d["t_obs"].shape[0]
    assert sh["n_theta"] >= 8 and sh["n_t"] >= 16 and (prm.theta_obs == 0 or n_phi_eff >= 2), sh
    assert n_phi_eff * sh["n_theta"] * sh["n_t"] <= 150000, "a model this large makes the long-double reference slow"
    st = [fr.FluxStage(fr.cells_from_cgs(d), prm.p, prm.z, prm.lumi_dist, prm.theta_obs, spreading)]
    if prm.flags & _lib.FLAG_RVS:
        st.append(fr.FluxStage(fr.cells_from_cgs(d, m.details(float(t_lo), float(t_hi), rvs=True)), prm.rvs_p, prm.z, prm.lumi_dist,
                               prm.theta_obs, spreading))
    if key is not None:
        _STAGES[ck] = (d, st)
    return d, st


def model(name):
    return _abi.make_params(**MODELS[name])


def nudge(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def standard_request(d, t_lo=T_LO, t_hi=T_HI, n_base=24):
    """Ascending times inside [t_lo, t_hi], both ends included (so every request of a window sees the same lattice): a log-spaced base
    plus nudge(t_node, k), k = -2 ... 2, for an interior node and the first node of three rows (lowest, middle, highest theta)."""
    t_obs = d["t_obs"]
    K = t_obs.shape[2]
    assert t_obs[:, :, -1].min() > t_hi, "a row ends inside the window: add the last-node sub-case"
    times = [np.geomspace(t_lo, t_hi, n_base)]
    for j in (0, t_obs.shape[1] // 2, t_obs.shape[1] - 1):
        for i in {0, t_obs.shape[0] - 1}:
            for node in (t_obs[i, j, K // 2], t_obs[i, j, 0]):
                times.append(np.array([nudge(node, k) for k in (-2, -1, 0, 1, 2)]))
    t = np.unique(np.concatenate(times))
    return t[(t >= t_lo) & (t <= t_hi)]


# ---- the metric ----
def metric(flux, got):
    """The maximum over the normal slots of |got - ref| / ref / max(1, |log2 ref| / 256); asserts the rules of tiny and zero slots."""
    got = np.asarray(got)
    ref = flux.nearest(got)
    reff = mr.to_float(ref)
    tiny = reff < 1e-250
    assert tiny.mean() <= 0.02, f"{tiny.mean():.1%} of the reference slots are below 1e-250"
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    assert np.all(got[reff == 0] == 0) and np.all(got[tiny] < 1e-250)
    ok = ~tiny
    with np.errstate(all="ignore"):
        scale = np.maximum(1.0, np.abs(np.log2(reff[ok])) / 256)
    return float(np.max(mr.to_float(np.abs(got[ok] - ref[ok]) / ref[ok]) / scale))


def record(form, name, err):
    m = MEASURED.get(form, {}).get(name)
    gate = None if m is None else GATE_FACTOR * m
    TABLE.append((form, name, err, gate))
    print(f"[flux stage] {form:26s} {name:16s} measured {err:.3e}  gate {gate}")
    return gate


def check(form, name, flux, got):
    err = metric(flux, got)
    gate = record(form, name, err)
    assert err < CEILING, f"{form} / {name}: {err:.3e} is above {CEILING:g}: a defect of the stage"
    assert gate is not None, f"{form} / {name}: measured {err:.3e}, no constant recorded"
    assert MEASURED[form][name] < CEILING and err <= gate, f"{form} / {name}: {err:.3e} > {gate:.3e}"


def grid_refs(st, t, nu):
    return [s.all_sides("grid", t, nu) for s in st]


def grid_got(eng, prm, t, nu):
    return list(dev_grid4(eng, prm, t, nu)) if prm.flags & _lib.FLAG_RVS else [dev_grid(eng, [prm], t, nu)[0]]


# ---- the lattice: vag_eat_details_kernel against the reference's ----
@pytest.mark.parametrize("name", sorted(MODELS))
def test_details_lattice(eng, name):
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    lat = st[0].lat
    t_ref = np.exp2(lat["lg2_t"]) / np.longdouble(mr.U_SEC)
    dop_ref = np.exp2(lat["lg2_doppler"])
    e_t = float(np.max(np.abs(d["t_obs"] - t_ref) / t_ref))
    e_d = float(np.max(np.abs(d["Doppler"] - dop_ref) / dop_ref))
    m = MEASURED_EAT.get(name)
    print(f"[flux stage] lattice {name:16s} shape {d['t_obs'].shape}  t_obs {e_t:.3e}  Doppler {e_d:.3e}  measured {m}")
    TABLE.append(("details t_obs", name, e_t, None if m is None else GATE_FACTOR * m[0]))
    TABLE.append(("details Doppler", name, e_d, None if m is None else GATE_FACTOR * m[1]))
    assert m is not None, f"{name}: t_obs {e_t:.3e}, Doppler {e_d:.3e}, no constant recorded"
    assert e_t <= min(GATE_FACTOR * m[0], EAT_CEILING) and e_d <= min(GATE_FACTOR * m[1], EAT_CEILING)


# ---- vag_flux_grid_kernel ----
GRID_FORMS = {
    "grid 256 one-item": (dict(VAG_FLUX_PERSISTENT="0"), "lanes=256", "one item"),
    "grid 256 persistent": (dict(VAG_FLUX_PERSISTENT="2"), "lanes=256", "persistent"),
    "grid 512 one-item": (dict(VAG_FLUX_PERSISTENT="0", VAG_FLUX_WIDE="1"), "lanes=512", "one item"),
    "grid 512 persistent": (dict(VAG_FLUX_PERSISTENT="2", VAG_FLUX_WIDE="1"), "lanes=512", "persistent"),
    "grid pieces of 8": (dict(VAG_FLUX_PERSISTENT="2", VAG_FLUX_K_CAP="8"), "ks=8 ", "persistent"),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_grid_kernel_forms(eng, capfd, name):
    """The standard request (edge times on the device's own nodes, a window most rows of the spreading model enter late, frequencies
    from far below nu_a into the cut-off) through every form of the workgroup kernel; a spreading model has its own instantiation
    (512 lanes), whose launch line the 256-lane forms' expectation is replaced by."""
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    t = standard_request(d)
    first = d["t_obs"][:, :, 0]
    if name == "gauss_spread":
        assert np.mean(first > T_LO) > 0.5, "premise: most rows' first node lies inside the window"
    assert np.any((first > T_LO) & (first < T_HI)) or prm.theta_obs == 0
    nu = NU_OF.get(name, NU4)
    assert t.size * nu.size <= 512
    refs = grid_refs(st, t, nu)
    parts = ["fwd", "rvs"]
    spreading = bool(prm.flags & _lib.FLAG_SPREADING)
    for form, (hooks, lanes, launch) in GRID_FORMS.items():
        with hooked(capfd, **hooks) as report:
            got = grid_got(eng, prm, t, nu)
            err = report()
        assert "grid flux form: " + launch in err, err
        if "pieces" in form:
            assert "ks=8 " in err and d["shape"]["n_t"] > 16, err  # pieces: times fall on both sides of more than one seam
        else:
            assert ("lanes=512" if spreading else lanes) in err, err
        for c, (ref, g) in enumerate(zip(refs, got)):
            check(form, name if len(refs) == 1 else f"{name}/{parts[c]}", ref, g)


@pytest.mark.parametrize("shape", [(1, 1), (128, 4), (171, 3)])
def test_grid_request_shapes(eng, capfd, shape):
    """nt = nnu = 1, and nt * nnu = 512 and 513: the last request the 256-lane form takes and the first it does not."""
    nt, nnu = shape
    name = "gauss_offaxis"
    prm = model(name)
    t = np.array([3e5]) if nt == 1 else np.geomspace(T_LO, T_HI, nt)
    nu = NU4[2:3] if nnu == 1 else NU4[:nnu]
    d, st = stages(prm, t[0], t[-1], name)
    with hooked(capfd) as report:
        got = dev_grid(eng, [prm], t, nu)[0]
        err = report()
    assert ("lanes=256" if nt * nnu <= 512 else "lanes=512") in err, err
    check(f"grid {nt}x{nnu}", name, st[0].all_sides("grid", t, nu), got)


# ---- vag_flux_series_kernel and vag_flux_fit_rows_kernel serving series ----
def series_request(d, n, nu_pool, rng, t_lo=T_LO, t_hi=T_HI):
    """n ascending times from the standard request (both ends kept), with repeated times, and frequencies drawn from nu_pool in
    shuffled order, so that (t, nu) pairs repeat and runs of equal frequency break off."""
    if n == 1:
        return np.array([3e5]), np.array([nu_pool[0]])
    base = standard_request(d, t_lo, t_hi, n_base=max(2, n // 3))
    inner = rng.choice(base[1:-1], size=n - 2, replace=True)
    t = np.sort(np.concatenate([[t_lo], inner, [t_hi]]))
    return t, rng.choice(nu_pool, size=n, replace=True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 512])
@pytest.mark.parametrize("name", ["gauss_offaxis", "tophat_onaxis"])
def test_series_forms(eng, capfd, name, n):
    """A series of n points through the three kernels that serve one: the row-per-lane fit kernel (few distinct frequencies, the
    product's choice), the wavefront-per-row series kernel on its shared-node path (VAG_SERIES_ROW_PER_WAVE, n <= 64) or per point
    (n > 64), and the per-point path the product takes for more than 8 distinct frequencies."""
    prm = model(name)
    rng = np.random.default_rng(n)
    d0, _ = stages(prm, T_LO, T_HI, name)
    t, nu = series_request(d0, n, NU4[:3], rng)
    d, st = stages(prm, t[0], t[-1], name)
    ref = st[0].all_sides("series", t, nu)
    few = n >= 6  # (upload_series_bands: sharing needs at least two points per distinct frequency)
    with hooked(capfd) as report:
        got = dev_series(eng, [prm], t, nu)[0]
        err = report()
    assert ("fit rows launch" in err) == few and ("series launch" in err) != few, err
    check("series fit-rows" if few else "series per-point", name, ref, got)
    with hooked(capfd, VAG_SERIES_ROW_PER_WAVE="1") as report:
        got = dev_series(eng, [prm], t, nu)[0]
        err = report()
    assert "series launch" in err and "fit rows launch" not in err, err
    shared = few and n <= 64
    assert (f"bands={np.unique(nu).size} " if shared else "bands=0 ") in err, err
    check("series shared-node" if shared else "series per-point", name, ref, got)
    if n >= 63:  # more than 8 distinct frequencies: the product's own per-point path
        nu_many = NU4[2] * np.exp2(rng.integers(-20, 21, size=n) / 2.0)
        with hooked(capfd) as report:
            got = dev_series(eng, [prm], t, nu_many)[0]
            err = report()
        assert "series launch" in err and "bands=0 " in err and "fit rows launch" not in err, err
        check("series per-point", name, st[0].all_sides("series", t, nu_many), got)


def test_series_with_a_point_in_the_far_cut_off(eng, capfd):
    """One of 64 points so far past nu_M that its flux underflows: it must be tiny (or 0 where the reference is) on the device too."""
    name = "gauss_offaxis"
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    t, nu = series_request(d, 64, NU4[:3], np.random.default_rng(7))
    nu[-1] = 1e30
    ref = st[0].all_sides("series", t, nu)
    assert mr.to_float(ref.value)[-1] < 1e-250
    with hooked(capfd):
        got = dev_series(eng, [prm], t, nu)[0]
    check("series fit-rows", name + "/cut-off", ref, got)


def test_spreading_series(eng, capfd):
    name = "gauss_spread"
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    t, nu = series_request(d, 64, NU4[:3], np.random.default_rng(5))
    ref = st[0].all_sides("series", t, nu)
    for form, hooks, line in (("series fit-rows", {}, "fit rows launch"), ("series shared-node", dict(VAG_SERIES_ROW_PER_WAVE="1"), "series launch")):
        with hooked(capfd, **hooks) as report:
            got = dev_series(eng, [prm], t, nu)[0]
            err = report()
        assert line in err, err
        check(form, name, ref, got)


def test_series_kernel_serving_a_grid(eng, capfd):
    """VAG_GRID_ROWWISE: the wavefront-per-row kernel on a (t, nu) grid."""
    name = "gauss_offaxis"
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    t = standard_request(d)
    with hooked(capfd, VAG_GRID_ROWWISE="1") as report:
        got = dev_grid(eng, [prm], t, NU4)[0]
        err = report()
    assert "series launch" in err and "grid flux launch" not in err, err
    check("grid by series kernel", name, st[0].all_sides("grid", t, NU4), got)


# ---- vag_flux_grid_rows_kernel: a (theta, phi) row per lane, for large batches of small grids ----
def test_grid_rows_kernel(eng, capfd):
    name = "gauss_offaxis"
    nb = 640  # x 506 rows: > 4096 blocks of 64 rows
    prms = jittered(MODELS[name], nb, seed=11)
    t, nu = np.geomspace(T_LO, T_HI, 32), NU4
    with hooked(capfd) as report:
        rows = dev_grid(eng, prms, t, nu)
        err = report()
    assert "grid rows launch" in err and "grid flux launch" not in err, err
    with hooked(capfd, VAG_GRID_ROW_PER_WORKGROUP="1") as report:
        wg = dev_grid(eng, prms, t, nu)
        err = report()
    assert "grid flux launch" in err and "grid rows launch" not in err, err
    for m in (0, nb // 2, nb - 1):
        d, st = stages(prms[m], t[0], t[-1])
        ref = st[0].all_sides("grid", t, nu)
        print(f"[flux stage] member {m} of {nb}:")
        check("grid rows (row per lane)", name + " batch", ref, rows[m])
        check("grid rows counterpart", name + " batch", ref, wg[m])


# ---- the band form ----
@pytest.mark.parametrize("name", ["gauss_offaxis", "gauss_spread"])
@pytest.mark.parametrize("num_nu", [5, 9])
def test_band_form(eng, capfd, name, num_nu):
    prm = model(name)
    d, st = stages(prm, T_LO, T_HI, name)
    t = standard_request(d)
    with hooked(capfd) as report:
        got = dev_band(eng, [prm], t, 1e14, 1e16, num_nu)[0]
        err = report()
    assert "grid flux launch" in err, err
    check(f"band of {num_nu}", name, st[0].all_sides("band", t, 1e14, 1e16, num_nu), got)


# ---- vag_flux_fit_rows_kernel through vag_loglike_batch ----
def test_loglike_of_the_fit_rows_kernel(eng, capfd):
    """ln L of a walker at the truth against the long-double ln L of the reference fluxes (vag_fit_back_kernel's formula:
    -1/2 sum w ((ln F_obs - ln F_model) / sigma)^2 with sigma = err / F_obs).  Every free parameter is on a linear scale, so the walker's
    model is bit for bit the model whose details were read.  ln L is compared relative to the number of rows -- the size of chi^2."""
    tr = configs.C4_TRUTH
    f = Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    fixed = dict(E_iso=tr["E_iso"], Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"])
    defs = [ParamDef("theta_c", 0.02, 0.3, Scale.linear), ParamDef("theta_v", 0.0, 0.8, Scale.linear), ParamDef("p", 2.05, 2.8, Scale.linear)]
    defs += [ParamDef(k, v, v, Scale.fixed, v) for k, v in fixed.items()]
    sample = np.array([[tr["theta_c"], tr["theta_obs"], tr["p"]]])
    t = np.sort(np.concatenate([configs.C4_EPOCHS] * 3))
    nu = np.tile(configs.C4_BANDS, configs.C4_EPOCHS.size)
    f.add_flux_density(1.0, [1.0], [1.0], [1.0])  # (a placeholder so that the spec can be built: replaced below)
    prm, _ = f._params_at(sample[0], defs)
    d, st = stages(prm, t[0], t[-1])
    ref = st[0].series(t, nu)
    assert not ref.alt
    ref_f = mr.to_ld(ref.value)
    rng = np.random.default_rng(2)
    obs = mr.to_float(ref_f) * (1 + 0.05 * rng.standard_normal(t.size))
    err_obs = 0.1 * obs
    f = Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    for band in configs.C4_BANDS:
        sel = nu == band
        f.add_flux_density(band, t[sel], obs[sel], err_obs[sel])
    f._consolidate_data()
    assert np.array_equal(f._all_t, t) and f._all_t.size <= 512
    with hooked(capfd) as report:
        got = f.loglike_batch(sample, defs)[0]
        err = report()
    assert "fit rows launch" in err, err
    # the fitter's rows in its own order, its own double ln F_obs, sigma and weights: only the model flux is the reference's
    order = [int(np.nonzero((t == tt) & (nu == nn))[0][0]) for tt, nn in zip(f._all_t, f._all_nu)]
    q = (f._all_log_flux.astype(np.longdouble) - np.log(ref_f[order])) / f._all_log_err.astype(np.longdouble)
    want = -0.5 * np.sum(f._all_weights.astype(np.longdouble) * q * q)
    rel = float(abs(np.longdouble(got) - want)) / t.size
    gate = record("loglike fit-rows", "gauss_offaxis", rel)
    print(f"[flux stage] ln L device {got!r}  reference {float(want)!r}  rows {t.size}")
    assert rel < CEILING
    assert gate is not None and rel <= gate
