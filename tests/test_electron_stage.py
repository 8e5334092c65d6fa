"""The device's synchrotron electron stage -- what turns (t_comv, Gamma_th, B, N_p, r) of a cell into gamma_M, gamma_m, gamma_c, N_e, the
column density, I_peak, nu_a, gamma_a and the break frequencies -- against the extended-precision reference of that stage alone
(tests/_elecref.py), link by link, every link fed with the DEVICE's own doubles of the link before.

Two producers of the device's values:
* the probe (vag_debug_device_math): VAG_MATH_ELEC_CELL calls syn_cell itself on chosen points -- 4096 log-uniform draws per p, 256
  relic cells, points placed on each threshold at -2 ... 2 ulps, the unshocked cell, p one ulp either side of 2 and 3 (the sets of
  _elecref.probe_set, the ones tests/test_electron_stage_host.py shows a float64 restatement to meet the ceilings on) -- and
  VAG_MATH_FWD_STATE calls fwd_shock_state, the function vag_cells_kernel finishes the forward shock's state with (link 0);
* Model.details of the five small models of tests/test_flux_stage.py: vag_cells_kernel's own wiring -- cell indexing, the crossing cell
  k_inj - 1 of a relic row, the reverse shock's own p, eps_e, xi_e -- forward shock of all five and the thick shell's reverse shock.
  A details call returns cgs values: they are brought back to code units here, which costs one more rounding per dimensional input.

Metric: the relative error of each of the eleven outputs under the link that produces it.  gamma_a is compared as gamma_a (gamma_a - 1 is
ill conditioned where nu_a is small, in the reference as much as on the device) and at the nearest branch the reference admits; at
p == 2 gamma_m is held to the bisection's own stop rule (_elecref.p2_bracket_holds) and everything after it is chained on the returned
gamma_m; an unshocked cell (B = 0) is compared by class and position with _elecref.unshocked_cell.

Gates: GATE_FACTOR x the maxima measured on an MI355X (MEASURED below), each of which must also stay under its ceiling
(_elecref.ceiling: ~25 x what IEEE double gives on the formula).  A figure that is missing has not been measured: its test fails after
printing the figure."""
import ctypes as C

import numpy as np
import pytest

import _abi
import _elecref as E
import _mathref as mr
import vegasafterglow_amd as va
from test_flux_stage import MODELS, T_HI, T_LO
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")
_dp = C.POINTER(C.c_double)

GATE_FACTOR = 4  # the suite's convention (DEVIANCE_GATE, tests/test_counts.py)
# (link, quantity, p class) -> the maximum relative error over the probe's sets, measured on an MI355X on 2026-10-19, rounded up to two
# digits.  Link 0's p class is None.
_C = ("p<2", "p=2", "2<p<=3", "p>3")


def _per_class(link, name, figures):
    return {(link, name, c): f for c, f in zip(_C, figures) if f is not None}


MEASURED_PROBE = {
    (0, "compression", None): 6.4e-16, (0, "Gamma_th", None): 1.7e-16, (0, "N_p", None): 1.1e-16, (0, "B", None): 2.4e-16,
    #                                  p < 2    p = 2    2 < p <= 3  p > 3
    **_per_class(1, "gamma_M",        (1.8e-16, 2.0e-16, 1.9e-16, 1.8e-16)),
    **_per_class(1, "gamma_m",        (1.2e-15, None,    2.7e-16, 3.3e-16)),  # (p = 2: the bisection's stop rule instead)
    **_per_class(1, "gamma_c",        (3.6e-16, 3.7e-16, 3.8e-16, 3.7e-16)),
    **_per_class(2, "N_e",            (2.3e-16, 2.4e-16, 2.6e-16, 3.5e-15)),
    **_per_class(2, "column_den",     (3.5e-16, 3.2e-16, 3.6e-16, 3.6e-15)),
    **_per_class(2, "I_nu_max",       (4.9e-16, 4.4e-16, 4.7e-16, 3.7e-15)),
    **_per_class(2, "gamma_a",        (7.9e-15, 7.2e-15, 7.0e-15, 8.2e-15)),
    **_per_class(3, "nu_m",           (2.8e-16, 2.8e-16, 3.0e-16, 2.9e-16)),
    **_per_class(3, "nu_c",           (2.7e-16, 2.9e-16, 2.8e-16, 2.8e-16)),
    **_per_class(3, "nu_a",           (3.1e-16, 3.0e-16, 2.8e-16, 2.9e-16)),
    **_per_class(3, "nu_M",           (2.6e-16, 2.5e-16, 2.5e-16, 2.5e-16)),
    **_per_class(3, "I_nu_max",       (2.6e-16, 2.7e-16, 2.7e-16, 2.5e-16)),
}
# (link, quantity) -> the same over the details of the five models (every one has 2 < p <= 3), forward and reverse shock; a details call
# returns no column density, so link 3's I_nu_max has no input there (link 2's is compared)
MEASURED_DETAILS = {
    (1, "gamma_M"): 2.3e-16, (1, "gamma_m"): 2.8e-16, (1, "gamma_c"): 7.3e-16,
    (2, "N_e"): 1.8e-16, (2, "I_nu_max"): 8.0e-16, (2, "gamma_a"): 5.5e-15,
    (3, "nu_m"): 4.3e-16, (3, "nu_c"): 4.1e-16, (3, "nu_a"): 4.5e-16, (3, "nu_M"): 3.6e-16,
}
TABLE = []


@pytest.fixture(scope="module")
def dev():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def run(name, x, n_out):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.full((x.shape[0], n_out), np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH_MORE[name], x.ctypes.data_as(_dp), x.shape[0], out.ctypes.data_as(_dp)))
        return out
    yield run
    lib.vag_ctx_destroy(ctx)
    if TABLE:
        print("\n[electron stage] source   link quantity    p class    measured   gate      ceiling")
        for src, link, name, cls, err, gate, ceil in TABLE:
            print(f"[electron stage] {src:8s} {link}    {name:11s} {str(cls):9s} {err:9.2e}  {gate if gate is None else format(gate, '.2e')}  {ceil:.0e}")


def hold(src, table, worst):
    """Every measured maximum against its ceiling and its gate; reports all before it fails on any."""
    bad = []
    for key, err in sorted(worst.items(), key=str):
        link, name, cls = key
        m = table.get(key if src == "probe" else key[:2])
        ceil = E.ceiling(link, name, cls)
        gate = None if m is None else GATE_FACTOR * m
        TABLE.append((src, link, name, cls, err, gate, ceil))
        print(f"[electron stage] {src} link {link} {name:11s} {str(cls):9s} measured {err:.3e}  gate {gate}  ceiling {ceil:.0e}")
        if not err <= ceil:
            bad.append(f"{key}: {err:.3e} is above the ceiling {ceil:g}: the device is wrong or the reference is")
        elif m is None:
            bad.append(f"{key}: measured {err:.3e}, no constant recorded")
        elif not (GATE_FACTOR * m <= ceil and err <= gate):
            bad.append(f"{key}: {err:.3e} > {gate:.3e}")
    assert not bad, "\n".join(bad)


def out_dict(out):
    return {n: out[:, i] for i, n in enumerate(E.OUT_NAMES)}


# ---------------------------------------------------------------- the probe: syn_cell
@pytest.fixture(scope="module")
def probed(dev):
    cache = {}

    def get(p):
        if p not in cache:
            rows, kind = E.probe_set(p)
            cache[p] = (rows, kind, dev("elec_cell", rows, 11))
        return cache[p]
    return get


@pytest.mark.parametrize("p", E.PS)
def test_probe_cells_against_the_reference(probed, p):
    rows, kind, out = probed(p)
    sh = kind != "unshocked"
    assert E.same_class(out[~sh][0], E.unshocked_cell(p)), out[~sh]
    r, k = rows[sh], kind[sh]
    assert np.all(np.isfinite(out[sh])), "a shocked probe row gives a non-finite output"
    e = E.chain_errors(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7], out_dict(out[sh]), r[:, 8] != 0,
                       (r[:, 9], r[:, 10], r[:, 11]))
    l2 = e["link2"]
    # the coverage condition, from the reference alone (on the device's gamma_m, gamma_c)
    drawn = np.isin(k, ("random", "relic", "steered"))
    counts = np.bincount(l2.branch[drawn], minlength=5)
    relic = r[:, 8] != 0
    print(f"[electron stage] p = {p}: {r.shape[0]} points, branches {counts.tolist()}, slow {int((l2.slow & drawn).sum())}, relic "
          f"{int((relic & drawn).sum())}, decided both ways: drawn {int(l2.both_ways[drawn].sum())}, placed "
          f"{int(l2.both_ways[k == 'placed'].sum())} of {int((k == 'placed').sum())}")
    assert counts.min() >= 100 and (l2.slow & drawn).sum() >= 100 and (~l2.slow & drawn).sum() >= 100
    assert (relic & drawn).sum() >= 100 and (~relic & drawn).sum() >= 100
    assert l2.both_ways[drawn].mean() <= 0.01
    assert np.all(e["p2_ok"]), "the device's bisection ends outside its own stop rule"
    hold("probe", MEASURED_PROBE, E.worst_by_class(e, r[:, 6]))


@pytest.mark.parametrize("n", [1, 63, 65])
def test_probe_gives_the_same_bits_whatever_the_launch(dev, probed, n):
    rows, kind, out = probed(2.3)
    assert np.array_equal(dev("elec_cell", rows[:n], 11), out[:n], equal_nan=True)
    sel = np.r_[rows.shape[0] - n:rows.shape[0]]  # (the set's tail: relic, placed and the unshocked row)
    assert np.array_equal(dev("elec_cell", rows[sel], 11), out[sel], equal_nan=True)


# ---------------------------------------------------------------- the probe: link 0
def test_forward_shock_state_against_the_reference(dev):
    rows = E.fwd_state_rows()
    out = dev("fwd_state", rows, 4)
    sh = rows[:, 3] != 0
    assert out[~sh].tolist() == [[1.0, 0.0, 0.0, 0.0]]
    r, o = rows[sh], out[sh]
    assert np.all(np.isfinite(o)) and np.all(o[r[:, 0] <= 1, 3] == 4.0)
    Gth, Np = E.link0_state(r[:, 2], r[:, 3])
    worst = {(0, "compression", None): E.rel(o[:, 3], E.compression(r[:, 0])).max(), (0, "Gamma_th", None): E.rel(o[:, 0], Gth).max(),
             (0, "N_p", None): E.rel(o[:, 2], Np).max(), (0, "B", None): E.rel(o[:, 1], E.link0_B(o[:, 0], o[:, 3], r[:, 1], r[:, 4])).max()}
    for n in (1, 63, 65):
        assert np.array_equal(dev("fwd_state", rows[-n:], 4), out[-n:])
    hold("probe", MEASURED_PROBE, {k: float(v) for k, v in worst.items()})


# ---------------------------------------------------------------- the kernel's wiring, through Model.details
def device_cells(name, rvs):
    prm = _abi.make_params(**MODELS[name])
    d = va.Model.from_params(prm).details(T_LO, T_HI, rvs=rvs)
    assert d["B"].size <= 150000
    rad = dict(p=prm.rvs_p, eps_e=prm.rvs_eps_e, xi_e=prm.rvs_xi_e) if rvs else dict(p=prm.p, eps_e=prm.eps_e, xi_e=prm.xi_e)
    cells = dict(t_comv=d["t_comv"] * mr.U_SEC, r=d["r"] * mr.U_CM, Gamma_th=d["Gamma_th"], B=d["B"] * E.U_GAUSS, N_p=d["N_p"])
    out = {n: d[n] for n in ("gamma_m", "gamma_c", "gamma_a", "gamma_M", "N_e")}
    out.update({n: d[n] * E.U_HZ for n in ("nu_m", "nu_c", "nu_a", "nu_M")})
    out["I_nu_max"] = d["I_nu_max"] * E.U_FLUX_DEN_CGS
    return prm, cells, out, rad


@pytest.mark.parametrize("name,rvs", [(n, False) for n in sorted(MODELS)] + [("rs_thick", True)])
def test_details_follow_the_chain(oracle, name, rvs):
    prm, cells, out, rad = device_cells(name, rvs)
    res = E.details_errors(cells, out, rad, rvs)
    nt = cells["B"].shape[1]
    print(f"[electron stage] {name}{'/rvs' if rvs else ''}: {res['n']} cells, {res['n_unshocked']} unshocked, {res['n_relic']} relic, "
          f"{res['n_degenerate']} with gamma_peak = 1")
    assert res["n"] - res["n_unshocked"] - res["n_degenerate"] > 0.5 * res["n"] and res["p2_ok"]
    if rvs:
        # one injection index per row, cells below it synchrotron-only, cells from it on cooled from cell k_inj - 1 (details_errors holds
        # both groups to link 1); the CPU checker's index, where its grid is the device's, is the same to a cell
        k_inj = res["k_inj"]
        assert np.all(k_inj >= 1) and np.any(k_inj < nt) and res["n_relic"] > 0
        want = oracle.details(prm, T_LO, T_HI, rvs=True)["injection_idx"][:, 0].astype(int)
        print(f"[electron stage]   injection index: device {k_inj.tolist()}  CPU checker {want.tolist()}")
        if want.shape == k_inj.shape:
            assert np.max(np.abs(np.minimum(want, nt) - k_inj)) <= 1
    else:
        assert res["n_relic"] == 0
    hold("details", MEASURED_DETAILS, res["worst"])


def test_write_back_variant_gives_the_same_bits():
    """vag_cells_kernel stores the finished Gamma_th, B, N_p only where something reads them again (a details call, the IC cooling pass);
    VAG_CELLS_WRITE_BACK turns the store on for a plain flux call: the same fluxes to the bit."""
    prm = _abi.make_params(**MODELS["gauss_offaxis"])
    t, nu = np.geomspace(T_LO, T_HI, 24), np.array([1e9, 4.84e14, 1e18])
    m = va.Model.from_params(prm)
    plain = m.flux_density_grid(t, nu).total
    _lib.hooks["VAG_CELLS_WRITE_BACK"] = "1"
    try:
        stored = m.flux_density_grid(t, nu).total
    finally:
        _lib.hooks.pop("VAG_CELLS_WRITE_BACK", None)
    assert np.all(np.isfinite(plain)) and plain.max() > 0
    assert np.array_equal(plain, stored)
