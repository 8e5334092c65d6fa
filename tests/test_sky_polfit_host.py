"""CPU tests of the polarization groups of the likelihood (vag_loglike_pol_batch, Fitter.add_polarization):

1. the ctypes layouts of vag_polarization_obs / vag_pol_fit_spec and the new constants against the C header, and the new symbols in
   _lib.EXPORTS and in the library built for gfx950;
2. Fitter.add_polarization checks its arguments;
3. build_spec maps the four pol_* names to their slots, fills the fixed values and the defaults of Model.sky_polarization, refuses
   pol_* parameters without polarization data and accepts "pa" with polarization data alone;
4. sharded likelihood calls refuse polarization data instead of dropping it."""
import ctypes as C
import os

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define O(f) offsetof(vag_polarization_obs, f)
#define S(f) offsetof(vag_pol_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_polarization_obs), O(nu), O(n), O(n_az), O(kind), O(pad), O(t),
           O(q), O(u), O(err_q), O(err_u), O(weight));
    printf("%zu %zu %zu %zu %zu\n", sizeof(vag_pol_fit_spec), S(n_groups), S(groups), S(b_fixed), S(pi_max_fixed));
    printf("%d %d %d %d %d %d %d\n", VAG_POL_QU, VAG_POL_DEGREE, VAG_POL_MAX_GROUPS, VAG_P_POL_B, VAG_P_POL_PI_MAX, VAG_P_POL_B_RVS,
           VAG_P_POL_PI_MAX_RVS);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O = _lib.PolarizationObs
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "nu", "n", "n_az", "kind", "pad", "t", "q", "u", "err_q", "err_u", "weight")]
    S = _lib.PolFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.groups.offset, S.b_fixed.offset,
                                                   S.pi_max_fixed.offset]
    assert [int(x) for x in lines[2].split()] == [_lib.POL_KINDS["qu"], _lib.POL_KINDS["degree"], 64] + [
        _lib.POL_SLOTS[n] for n in ("pol_b", "pol_pi_max", "pol_b_rvs", "pol_pi_max_rvs")]
    assert [_lib.POL_SLOTS[n] for n in ("pol_b", "pol_pi_max", "pol_b_rvs", "pol_pi_max_rvs")] == [1004, 1005, 1006, 1007]


def test_new_symbols_exported():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_pol_batch", "vag_loglike_pol_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s


def _fitter(**kw):
    f = fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)
    f.add_flux_density(3e9, [1e6, 3e6], [1e-27, 2e-27], [1e-28, 2e-28])
    return f


def _group():
    t = np.array([6.5e6, 1.4e7, 2e7, 3.5e7])
    return dict(nu=3e9, t=t, q=np.array([0.14, 0.16, 0.15, 0.11]), u=np.array([0.01, -0.02, 0.0, 0.03]), err_q=np.full(4, 0.01),
                err_u=np.full(4, 0.02))


def _add(f, a, **kw):
    f.add_polarization(a["nu"], a["t"], a["q"], a.get("u"), a.get("err_q"), a.get("err_u"), **kw)


def test_add_polarization_stores_the_group():
    f = fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism")
    assert not f.has_polarization
    with pytest.raises(ValueError, match="add_polarization"):
        f.build_spec([fitting.ParamDef("theta_v", 0.0, 0.8)])  # the "no data" message names the new method
    a = _group()
    _add(f, a, weights=np.arange(4.0), n_az=64)
    f.add_polarization(a["nu"], a["t"], np.abs(a["q"]), err_q=a["err_q"], kind="degree")
    assert f.has_polarization and len(f._pol_obs) == 2
    pd = f._pol_obs[0]
    assert np.array_equal(pd["q"], a["q"]) and np.array_equal(pd["err_u"], a["err_u"]) and np.array_equal(pd["weights"], np.arange(4.0))
    assert pd["n_az"] == 64 and pd["kind"] == "qu"
    deg = f._pol_obs[1]
    assert deg["u"] is None and deg["err_u"] is None and deg["n_az"] is None and np.all(deg["weights"] == 1)
    spec, _, _ = f.build_spec([fitting.ParamDef("theta_v", 0.0, 0.8)])  # a fit with polarization data only
    assert spec.n_data == 0 and spec._pol.n_groups == 2 and spec._vis is None and spec._sky.n_groups == 0
    g = spec._pol.groups[0]
    assert (g.nu, g.n, g.n_az, g.kind) == (3e9, 4, 64, 0)
    assert g.t[3] == 3.5e7 and g.q[1] == 0.16 and g.u[1] == -0.02 and g.err_u[0] == 0.02 and g.weight[3] == 3.0
    g = spec._pol.groups[1]
    assert (g.n_az, g.kind) == (0, 1) and not g.u and not g.err_u and g.q[0] == 0.14


def test_add_polarization_argument_errors():
    f = _fitter()
    a = _group()
    _add(f, a)  # valid
    nan = np.array([1, 1, 1, np.nan])
    bad = [
        dict(nu=-1.0), dict(nu=np.nan), dict(nu=[3e9, 4e9]), dict(nu=0.0),
        dict(t=a["t"][:3]), dict(q=np.zeros(3)), dict(u=np.zeros(5)), dict(err_q=a["err_q"][:2]), dict(err_u=a["err_u"][:3]),
        dict(t=a["t"][::-1].copy()), dict(t=np.array([0.0, 1e6, 2e6, 3e6])), dict(t=a["t"].reshape(2, 2)),
        dict(t=a["t"] * np.array([1, 1, 1, np.inf])),
        dict(q=a["q"] * nan), dict(u=a["u"] * nan), dict(err_q=a["err_q"] * nan), dict(err_u=a["err_u"] * nan),
        dict(err_q=np.array([0.01, 0.01, 0.01, 0.0])), dict(err_u=-a["err_u"]),
        dict(q=np.array([0.1, 0.1, 0.1, 1.5])), dict(u=np.array([0.1, -1.01, 0.1, 0.1])),
        dict(weights=np.array([1.0, 1.0, 1.0, -1.0])), dict(weights=np.ones(3)), dict(weights=nan),
        dict(u=None), dict(err_u=None), dict(err_q=None),
        dict(kind="degree"),  # a negative degree: q[..] of _group is fine, so make one negative
        dict(kind="stokes"), dict(n_az=0), dict(n_az=-4), dict(n_az=2.5),
        dict(t=np.array([]), q=np.array([]), u=np.array([]), err_q=np.array([]), err_u=np.array([])),
    ]
    for kw in bad:
        b = dict(a)
        b.update({k: v for k, v in kw.items() if k in a})
        extra = {k: v for k, v in kw.items() if k not in a}
        if kw == dict(kind="degree"):
            b["q"] = np.array([0.1, -0.1, 0.1, 0.1])
        with pytest.raises(ValueError, match="add_polarization"):
            _add(f, b, **extra)
    with pytest.raises(ValueError, match="add_polarization"):
        f.add_polarization(3e9, a["t"], np.array([0.1, 0.2, 1.2, 0.1]), err_q=a["err_q"], kind="degree")  # a degree > 1
    assert len(f._pol_obs) == 1
    f.add_polarization(3e9, a["t"], np.array([0.0, 0.2, 1.0, 0.1]), err_q=a["err_q"], kind="degree")  # u, err_u not needed
    assert len(f._pol_obs) == 2


def test_build_spec_slots_defaults_and_fixed_values():
    S = fitting.Scale
    f = _fitter(rvs_shock=True)
    free = [fitting.ParamDef("theta_v", 0.0, 0.8), fitting.ParamDef("pol_b", 0.0, 3.0), fitting.ParamDef("pol_pi_max", 0.1, 1.0, S.log),
            fitting.ParamDef("pol_b_rvs", 0.0, 3.0), fitting.ParamDef("pol_pi_max_rvs", 0.0, 1.0), fitting.ParamDef("pa", -3.2, 3.2)]
    for defs in (free, free[:2], [free[0], fitting.ParamDef("pol_b_rvs", 0.5, 0.5, S.fixed)]):
        with pytest.raises(ValueError, match="add_polarization"):
            f.build_spec(defs)  # pol_* without polarization data
        with pytest.raises(ValueError, match="add_polarization"):
            f.validate_parameters(defs)
    with pytest.raises(ValueError, match="centroid"):
        f.build_spec([free[0], free[5]])  # no sky data at all: the message of the centroid and visibility groups
    _add(f, _group())
    f.validate_parameters(free)
    spec, lower, upper = f.build_spec(free)
    assert list(spec.slot[:6]) == [_lib.PARAM_SLOTS["theta_v"], 1004, 1005, 1006, 1007, 1001]
    assert list(spec.is_log[:6]) == [0, 0, 1, 0, 0, 0] and lower[2] == -1.0 and upper[2] == 0.0
    assert spec._pol.n_groups == 1 and spec._vis is None
    assert spec._sky is not None and spec._sky.n_groups == 0 and spec._sky.pa_fixed == 0.0
    # the defaults of Model.sky_polarization: b = 0, the reverse shock follows the forward b, pi_max from the walker's own p
    plain, _, _ = f.build_spec(free[:1])
    assert list(plain._pol.b_fixed) == [0.0, -1.0] and list(plain._pol.pi_max_fixed) == [-1.0, -1.0]
    fixed = [free[0], fitting.ParamDef("pol_b", 0.5, 0.5, S.fixed), fitting.ParamDef("pol_pi_max", 0.7, 0.7, S.fixed),
             fitting.ParamDef("pol_b_rvs", 2.0, 2.0, S.fixed), fitting.ParamDef("pol_pi_max_rvs", 0.6, 0.6, S.fixed),
             fitting.ParamDef("pa", 0.3, 0.3, S.fixed)]
    spec, _, _ = f.build_spec(fixed)
    assert spec.ndim == 1 and list(spec._pol.b_fixed) == [0.5, 2.0] and list(spec._pol.pi_max_fixed) == [0.7, 0.6]
    assert spec._sky.pa_fixed == 0.3
    for name, value in (("pol_b", -0.5), ("pol_pi_max", 1.5), ("pol_b_rvs", np.nan)):
        with pytest.raises(ValueError, match=name):
            f.build_spec([free[0], fitting.ParamDef(name, value, value, S.fixed)])
    p, _ = f._params_at([0.3, 0.5, -0.2, 1.0, 0.5, 1.0], free)  # none of them is a Model field
    assert p.theta_obs == 0.3


def test_pa_alone_with_polarization_data():
    f = _fitter()
    _add(f, _group())
    defs = [fitting.ParamDef("theta_v", 0.0, 0.8), fitting.ParamDef("pa", -3.2, 3.2)]
    spec, _, _ = f.build_spec(defs)
    assert list(spec.slot[:2]) == [_lib.PARAM_SLOTS["theta_v"], 1001] and spec._pol.n_groups == 1
    for name in ("east0", "north0"):  # these place centroid and visibility groups only
        with pytest.raises(ValueError, match="centroid"):
            f.build_spec(defs + [fitting.ParamDef(name, -1e-9, 1e-9)])
    f.add_centroid(3e9, [1e6], [0.0], [0.0], [1e-9], [1e-9])
    spec, _, _ = f.build_spec(defs + [fitting.ParamDef("east0", -1e-9, 1e-9)])
    assert spec._sky.n_groups == 1 and spec._pol.n_groups == 1 and spec.slot[2] == 1002


def test_sharded_calls_refuse_polarization_data():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_polarization = True
    with pytest.raises(NotImplementedError, match="add_polarization"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    _add(f, _group())
    with pytest.raises(NotImplementedError, match="add_polarization"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
