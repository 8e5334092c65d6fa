"""CPU tests of the visibility groups of the likelihood (vag_loglike_vis_batch, Fitter.add_visibilities):

1. the ctypes layouts of vag_visibility_obs / vag_vis_fit_spec against the C header, and the new symbols in _lib.EXPORTS and in the
   library built for gfx950;
2. Fitter.add_visibilities checks its arguments, finds the epochs from runs of equal t and builds first[] for ragged epochs;
3. build_spec with visibility data only accepts the sky parameters and maps them to their slots; without sky data it raises as before;
4. sharded likelihood calls refuse visibility data instead of dropping it."""
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
#define O(f) offsetof(vag_visibility_obs, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_visibility_obs), O(nu), O(n_epochs), O(n_vis), O(n_az),
           O(kind), O(t), O(first), O(u), O(v), O(re), O(im), O(err), O(weight));
    printf("%zu %zu %zu\n", sizeof(vag_vis_fit_spec), offsetof(vag_vis_fit_spec, n_groups), offsetof(vag_vis_fit_spec, groups));
    printf("%d %d %d %d %d\n", VAG_VIS_COMPLEX, VAG_VIS_AMPLITUDE, VAG_VIS_MAX_PER_EPOCH >= VAG_SKY_MAX_BASELINES, VAG_VIS_MAX_EPOCHS >= 1,
           VAG_VIS_MAX_GROUPS >= 1);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O = _lib.VisibilityObs
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "nu", "n_epochs", "n_vis", "n_az", "kind", "t", "first", "u", "v", "re", "im", "err", "weight")]
    S = _lib.VisFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.groups.offset]
    assert [int(x) for x in lines[2].split()] == [_lib.VIS_KINDS["complex"], _lib.VIS_KINDS["amplitude"], 1, 1, 1]


def test_new_symbols_exported():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_vis_batch", "vag_loglike_vis_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s


def _fitter():
    f = fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism")
    f.add_flux_density(3e9, [1e6, 3e6], [1e-27, 2e-27], [1e-28, 2e-28])
    return f


def _group():
    t = np.array([1e6, 1e6, 1e6, 2e7, 3e7, 3e7])
    u = np.array([1e6, -2e6, 3e6, 4e6, 5e6, -6e6])
    v = np.array([0.0, 1e6, 2e6, -3e6, 4e6, 5e6])
    vis = np.array([1 + 1j, 2 - 1j, 0.5j, 1.0, -1 - 1j, 2.0]) * 1e-27
    err = np.full(6, 1e-28)
    return dict(nu=8e9, t=t, u=u, v=v, vis=vis, err=err)


def _add(f, a, **kw):
    f.add_visibilities(a["nu"], a["t"], a["u"], a["v"], a["vis"], a["err"], **kw)


def test_epochs_are_runs_of_equal_times():
    f = fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism")
    assert not f.has_visibilities
    a = _group()
    _add(f, a, weights=np.arange(6.0), n_az=64)
    _add(f, dict(a, vis=np.abs(a["vis"])), kind="amplitude")
    assert f.has_visibilities and len(f._vis_obs) == 2
    vd = f._vis_obs[0]
    assert np.array_equal(vd["t"], [1e6, 2e7, 3e7]) and np.array_equal(vd["first"], [0, 3, 4, 6]) and vd["first"].dtype == np.int32
    assert np.array_equal(vd["re"] + 1j * vd["im"], a["vis"]) and np.array_equal(vd["weights"], np.arange(6.0))
    assert vd["n_az"] == 64 and vd["kind"] == "complex"
    amp = f._vis_obs[1]
    assert amp["im"] is None and amp["n_az"] is None and np.array_equal(amp["re"], np.abs(a["vis"])) and np.all(amp["weights"] == 1)
    spec, _, _ = f.build_spec([fitting.ParamDef("theta_v", 0.0, 0.8)])  # a fit with visibility data only
    assert spec.n_data == 0 and spec._vis.n_groups == 2
    g = spec._vis.groups[0]
    assert (g.nu, g.n_epochs, g.n_vis, g.n_az, g.kind) == (8e9, 3, 6, 64, 0)
    assert [g.first[i] for i in range(4)] == [0, 3, 4, 6] and g.t[2] == 3e7 and g.u[5] == -6e6 and g.im[1] == -1e-27
    g = spec._vis.groups[1]
    assert (g.n_az, g.kind) == (0, 1) and not g.im


def test_add_visibilities_argument_errors():
    f = _fitter()
    a = _group()
    _add(f, a)  # valid
    nan = np.array([1, 1, 1, 1, 1, np.nan])
    bad = [
        dict(nu=-1.0), dict(nu=np.nan), dict(nu=[8e9, 9e9]), dict(nu=0.0),
        dict(t=a["t"][:5]), dict(u=np.zeros(5)), dict(v=np.zeros(7)), dict(vis=a["vis"][:5]), dict(err=a["err"][:3]),
        dict(t=a["t"][::-1].copy()), dict(t=np.array([0.0, 1e6, 1e6, 2e7, 3e7, 3e7])), dict(t=a["t"].reshape(2, 3)),
        dict(u=a["u"] * nan), dict(v=a["v"] * nan), dict(vis=a["vis"] * nan), dict(vis=a["vis"] * (1 + 1j * np.inf)),
        dict(err=np.array([1e-28] * 5 + [0.0])), dict(err=-a["err"]), dict(err=a["err"] * nan),
        dict(weights=np.array([1.0] * 5 + [-1.0])), dict(weights=np.ones(5)), dict(weights=nan),
        dict(kind="amplitude"),  # complex data
        dict(kind="phase"), dict(n_az=0), dict(n_az=-4), dict(n_az=2.5),
        dict(t=np.array([]), u=np.array([]), v=np.array([]), vis=np.array([]), err=np.array([])),
    ]
    for kw in bad:
        b = dict(a)
        b.update({k: v for k, v in kw.items() if k in a})
        extra = {k: v for k, v in kw.items() if k not in a}
        with pytest.raises(ValueError):
            _add(f, b, **extra)
    assert len(f._vis_obs) == 1


def test_sky_parameters_with_visibility_data_only():
    f = _fitter()
    defs = [fitting.ParamDef("theta_v", 0.0, 0.8), fitting.ParamDef("pa", -3.2, 3.2), fitting.ParamDef("east0", -1e-9, 1e-9),
            fitting.ParamDef("north0", 2e-10, 2e-10, fitting.Scale.fixed)]
    with pytest.raises(ValueError, match="centroid"):
        f.build_spec(defs)  # neither centroid nor visibility data yet
    _add(f, _group())
    f.validate_parameters(defs)
    spec, _, _ = f.build_spec(defs)
    assert list(spec.slot[:3]) == [_lib.PARAM_SLOTS["theta_v"], 1001, 1002]
    assert spec._vis.n_groups == 1
    assert spec._sky.n_groups == 0 and spec._sky.north0_fixed == 2e-10 and spec._sky.pa_fixed == 0.0  # the fixed placement alone
    p, _ = f._params_at([0.3, 1.0, 0.0], defs)  # the sky placement is not a Model field
    assert p.theta_obs == 0.3
    plain, _, _ = _fitter().build_spec(defs[:1])
    assert plain._sky is None and plain._vis is None


def test_sharded_calls_refuse_visibility_data():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_visibilities = True
    with pytest.raises(NotImplementedError, match="add_visibilities"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    _add(f, _group())
    with pytest.raises(NotImplementedError, match="add_visibilities"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
