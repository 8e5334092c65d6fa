"""What lies between the pair solver's raw ODE state and the reverse-shock cells (Gamma_th, B, N_p), on the device, against the
extended-precision reference of that code alone (tests/_rsref.py): the closed forms rel_Gamma, downstr_4vel, jump_4vel, sound_speed and
their fast forms, rvs_shock_state, rvs_cross_state, rvs_early_extrap, CrossLattice and PairShock::init_state, each through its probe
routine (vag_debug_device_math) on the probe set tests/test_reverse_state_host.py shows a float64 restatement to meet the ceilings on.
The ODE right-hand side and the integrator stay held end to end (tests/test_gpu_parity.py, 2e-6 against the CPU checker).

Metric: the relative error of the returned value under the nearest reference the thresholds admit, per quantity and class (gamma_rel - 1
below 1e-3 or not; sigma at or below SIGMA_CUT, within a decade above it, beyond).  Gates: GATE_FACTOR x the maxima measured on an
MI355X (MEASURED below), each of which must itself stay under its ceiling (_rsref.ceiling: 25 x what IEEE double gives on the formula;
for |fast - exact| the bound from rcp1's and sqrt1's own figures).  A figure that is missing has not been measured: its test fails after
printing it."""
import ctypes as C

import numpy as np
import pytest

import _rsref as R
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")
_dp = C.POINTER(C.c_double)

GATE_FACTOR = 4  # the suite's convention (tests/test_electron_stage.py)
# (quantity, class ...) -> the maximum over the probe set, measured on an MI355X on 2026-10-21, rounded up to two digits
MEASURED = {
    ("rel_Gamma",): 2.5e-16, ("sound_speed",): 4.0e-16,
    #                        hydro    near-cut  magnetised
    **R._by_class("u_down", ((5.0e-16, 8.0e-12, 4.5e-09),      # gamma_rel - 1 < 1e-3
                             (8.3e-16, 8.0e-16, 5.4e-15))),    # gamma_rel - 1 >= 1e-3
    **R._by_class("jump",   ((4.5e-16, 5.9e-16, 5.4e-16),
                             (5.3e-16, 6.2e-16, 5.2e-16))),
    ("|rel_Gamma_f - rel_Gamma|",): 8.2e-16, ("|sound_speed_f - sound_speed|",): 4.0e-15,
    ("|jump_f - jump|", "g<1e-3"): 2.9e-15, ("|jump_f - jump|", "g>=1e-3"): 9.8e-16,
    ("rvs.Gamma_th",): 1.8e-16, ("rvs.N_p",): 1.1e-16, ("rvs.V3_comv",): 2.1e-16,
    **R._by_class("rvs.B",          ((1.1e-15, 1.4e-05, 9.1e-07),
                                     (5.9e-16, 4.6e-11, 2.7e-12))),
    **R._by_class("rvs.rho3",       ((7.0e-16, 1.4e-05, 2.0e-06),
                                     (6.0e-16, 1.3e-13, 8.2e-14))),
    **R._by_class("rvs.B3_ordered", ((0.0,     1.4e-05, 2.0e-06),
                                     (0.0,     8.6e-11, 4.7e-12))),
    ("lattice.node",): 3.5e-15,
    ("extrap.Gamma_th",): 1.2e-16, ("extrap.B",): 1.4e-12, ("extrap.N_p",): 4.0e-12,
    ("init.Gamma",): 3.0e-15, ("init.x4",): 4.8e-16, ("init.x3",): 4.8e-16, ("init.m2",): 5.7e-15, ("init.U2",): 7.8e-15,
    ("init.r",): 5.4e-16, ("init.t_comv",): 4.4e-16, ("init.eps4",): 1.1e-16, ("init.m4",): 1.1e-16,
    ("init.m3", "hydro"): 2.2e-15, ("init.m3", "near-cut"): 2.2e-06, ("init.m3", "magnetised"): 4.2e-07,
    ("init.U3", "hydro"): 1.8e-15, ("init.U3", "near-cut"): 4.2e-15, ("init.U3", "magnetised"): 3.1e-15,
}
TABLE = []


@pytest.fixture(scope="module")
def dev():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    cache = {}

    def run(name, rows=None):
        """The probe routine on rows (default: its probe set, evaluated once)."""
        if rows is None and name in cache:
            return cache[name]
        x = np.ascontiguousarray(R.probe_set(name)[0] if rows is None else rows, dtype=np.float64)
        n_in, n_out = _lib.MATH_RS_SHAPES[name]
        assert x.shape[1] == n_in
        out = np.full((x.shape[0], n_out), np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH_MORE[name], x.ctypes.data_as(_dp), x.shape[0], out.ctypes.data_as(_dp)))
        if rows is None:
            cache[name] = out
        return out
    yield run
    lib.vag_ctx_destroy(ctx)
    if TABLE:
        print("\n[reverse state] quantity, class                              measured   gate      ceiling")
        for key, err, gate, ceil in TABLE:
            print(f"[reverse state] {' '.join(key):44s} {err:9.2e}  {gate if gate is None else format(gate, '.2e')}  {ceil:.1e}")


def hold(worst):
    """Every measured maximum against its ceiling and its gate; reports all before it fails on any."""
    bad = []
    for key, err in sorted(worst.items()):
        m = MEASURED.get(key)
        ceil = R.ceiling(*key)
        gate = None if m is None else GATE_FACTOR * m
        TABLE.append((key, err, gate, ceil))
        print(f"[reverse state] {' '.join(key):44s} measured {err:.3e}  gate {gate}  ceiling {ceil:.1e}")
        if not err <= ceil:
            bad.append(f"{key}: {err:.3e} is above the ceiling {ceil:g}: the device is wrong or the reference is")
        elif m is None:
            bad.append(f"{key}: measured {err:.3e}, no constant recorded")
        elif key in R.FAST_BOUNDS:
            # the ceiling of a |fast - exact| is a bound, not 25 x a figure: the device reaches 20 % to 60 % of it (one sqrt1 alone is
            # 4.15e-15 of sound_speed_f's 6.8e-15), so 4 x measured would pass it.  The gate is the smaller of the two.
            if not err <= min(gate, ceil):
                bad.append(f"{key}: {err:.3e} > {min(gate, ceil):.3e}")
        elif not (gate <= ceil and err <= gate):
            bad.append(f"{key}: {err:.3e} > {gate:.3e}, or the gate is above the ceiling {ceil:.1e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["rel_gamma", "shock_jump", "sound_speed", "rvs_state", "rvs_extrap", "pair_init"])
def test_probe_routine_against_the_reference(dev, name):
    out = dev(name)
    assert np.all(np.isfinite(out)), "a probe row gives a non-finite output"
    worst, counts = R.errors(name, out)
    assert not any(counts.values()), counts
    hold(worst)


def test_lattices_integers_exactly_and_nodes_ascending(dev):
    lats = R.lattice_set()
    rows, owner = R.probe_set("cross_lattice")
    out = dev("cross_lattice")
    made = []
    for j, lat in enumerate(lats):
        o = out[owner == j]
        assert o.shape[0] == lat[4] and np.all(o[:, 1:] == o[0, 1:]), "one lattice, two sets of integers"
        made.append(dict(n_pre=o[0, 1], n_post=o[0, 2], plain=o[0, 3], nodes=o[:, 0]))
        assert o[0, 0] == pytest.approx(lat[0], rel=1e-14) and o[-1, 0] == pytest.approx(lat[1], rel=1e-14)
    worst, problems = R.lattice_errors(lats, made)  # the integers of some admitted reference, exactly; strictly ascending nodes
    assert not problems, "\n".join(problems)
    # away from a threshold the reference admits one set of integers: the float64 restatement's
    for lat, m in zip(lats, made):
        if len({(v["n_pre"], v["n_post"], v["plain"]) for v in R.lattice_variants(lat)}) == 1:
            f = R.f64_lattice(*lat)
            assert (int(m["n_pre"]), int(m["n_post"]), int(m["plain"])) == (f["n_pre"], f["n_post"], f["plain"])
    hold({("lattice.node",): worst})


@pytest.mark.parametrize("n", [1, 63, 65])
def test_probe_gives_the_same_bits_whatever_the_launch(dev, n):
    for name in _lib.MATH_RS_SHAPES:
        rows, full = R.probe_set(name)[0], dev(name)
        assert np.array_equal(dev(name, rows[:n]), full[:n]) and np.array_equal(dev(name, rows[-n:]), full[-n:]), name
