"""The twenty-two likelihood entry points (vag_loglike_{,sky_,vis_,pol_,lim_,noise_,counts_,index_,fold_,tmpl_,cov_}batch and their _dev
forms) are one request path: a request whose optional blocks are absent or empty is the narrower entry point's request, bit for bit; the host form
is the device-pointer form; a call does not depend on the evaluation order; an invalid walker scores -inf through the back kernels'
shared closing block and leaves the others alone.

Three fixtures, all on C4 (configs.C4_TRUTH): (a) the 60 point rows alone; (b) one fitter with every kind of data the first sixteen
entry points take; (c) the same plus a count spectrum, a template and two correlated groups: every kind of data the likelihood takes,
through the widest entry point.  Two batch sizes: 3 walkers (evaluated in the identity order) and 64, the smallest batch evaluated in cost order.
profiles/loglike_bits.py writes ln L of the same fixtures to a file, to compare two builds."""
import copy
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_cov as tcov
import test_fold as tf
import test_index as ti
import test_limits as tl
import test_sky_polfit as tp
import test_sky_visfit as tv
import test_templates as tt
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
P = fitting.ParamDef
BATCHES = (3, 64)
DAY = 86400.0


def fixture_a():
    """The C4 point data (60 rows): the device's own truth with 5 % noise, 10 % errors.  Returns (fitter, parameter list)."""
    t, nu = configs.c4_mock_data()
    truth = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], t, nu)[0]
    obs = truth * (1 + 0.05 * np.random.default_rng(42).standard_normal(t.size))
    f = tc.new_fitter()
    f.add_flux_density(nu, t, obs, 0.1 * truth)
    return f, tl.defs()


def fixture_b(other=False):
    """One fitter with a point block (8 rows at 3 GHz, plus 4 rows at 5 GHz in the noise group "a" with a calibration term, one of
    them a limit row), a band group with a limit row, a centroid group, a visibility group, a degree-polarization group with a limit
    epoch, a counts group and a spectral-index group: 2 to 4 epochs each, built by the helpers of the tests of each kind.  Free:
    theta_c, theta_v, E_iso, pa, east0, pol_b, sys_a.  other: the same shapes with other values -- the centroids' east coordinate
    shifted by 0.1 mas, the visibilities' real parts scaled by 1.1, the polarization degrees by 0.9.  Returns (fitter, parameter
    list)."""
    f = tv._c4_fitter(with_centroid=True, east0_true=tv.EAST0_TRUE + (0.1 * tv.units.mas if other else 0.0))  # 8 point rows, 3 centroid epochs
    truth = tv._c4_truth()
    rng = np.random.default_rng(7)
    t4 = np.array([20.0, 60.0, 150.0, 260.0]) * DAY
    f4 = truth.flux_density_grid(t4, 5e9).total[0]
    lim4 = np.array([False, True, False, False])
    f.add_flux_density(5e9, t4, np.where(lim4, 1.3 * f4, f4 * (1 + 0.05 * rng.standard_normal(4))), 0.1 * f4, upper_limit=lim4,
                       noise="a", calibration=0.05)
    bt = tc.EPOCHS[2::6]  # 3 epochs
    bflux = tc.device_flux([_abi.make_params(**configs.C4_TRUTH)], bt, tl.BAND, 7)[0]
    blim = np.array([False, False, True])
    f.add_flux(tl.BAND, bt, np.where(blim, 1.2 * bflux, bflux * (1 + 0.05 * rng.standard_normal(3))), 0.1 * bflux, num_points=7,
               upper_limit=blim)
    vd = tv.make_group(truth, tv.VIS_T, tv.VIS_NU, (4, 3, 5), tv.PA_TRUE, tv.EAST0_TRUE)
    tv.add_group(f, vd[:3] + (vd[3] + 0.1 * vd[3].real,) + vd[4:] if other else vd, n_az=64)
    pol = tp.make_group(truth)  # 4 epochs
    degree = np.hypot(pol["q"], pol["u"]) * (0.9 if other else 1.0)
    plim = np.array([False, True, False, False])
    f.add_polarization(pol["nu"], pol["t"], np.where(plim, degree + 0.02, degree), err_q=pol["err"], kind="degree",
                       weights=[1.0, 0.5, 2.0, 1.5], upper_limit=plim)
    f.add_counts(**tc.make_group(tc.EPOCHS[3::6], np.full(3, 5e4), 1, seed=11))
    f.add_spectral_index(**ti.make_group(ti.X_BAND, tc.EPOCHS[1::6], 2, "photon", seed=31))
    d = tv.FLUX_DEFS + tv.SKY_DEFS + [tp.POL_DEFS[1], P("sys_a", 0.0, 0.2)] + tv._c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    return f, d


def fixture_c():
    """Fixture (b)'s fitter plus the three kinds it lacks: a count-spectrum group (4 bins, 2 channels, 3 epochs, with a cross-section:
    N_H is read), 3 point rows at 8 GHz that carry the template "sn", and two correlated groups of 2 and 65 rows (each side of the
    64-lane stride), built by the helpers of the tests of each kind.  Free on top of (b): amp_sn, N_H.  Returns (fitter, parameter
    list)."""
    f, d = fixture_b()
    truth_n_h, d_n_h = np.append(tc.TRUTH, tf.LOG_N_H_TRUE), tf.defs(tf.N_H_DEF)
    f.add_count_spectrum(**tf.make_group(4, 2, tc.EPOCHS[4::6], np.full(3, 4e4), 1, seed=51, absorption=True, truth=truth_n_h, d=d_n_h))
    t3 = np.array([40.0, 70.0, 120.0]) * DAY
    f3 = tv._c4_truth().flux_density_grid(t3, 8e9).total[0]
    bump = tt.sn_bump(t3)
    f.add_flux_density(8e9, t3, f3 * (1 + 0.3 * bump), 0.1 * f3, templates={"sn": f3.max() * bump})
    for n, kind in ((2, "cal"), (65, "gp")):
        f.add_correlated(**tcov.make_data(n, kind))
    free = len(tv.FLUX_DEFS + tv.SKY_DEFS) + 2
    return f, d[:free] + [P("amp_sn", 0.0, 1.0)] + tf.N_H_DEF + d[free:]


def extra_groups():
    """A second group, of another row count than fixture (c)'s one, for each of the seven list kinds of which (c) holds one group:
    a band group (2 rows for 3), a centroid group (2 epochs for 3), a visibility group (5 visibilities in 2 epochs for 12 in 3), a
    QU polarization group (3 epochs for 4), a counts group (2 rows for 3), a spectral-index group (4 rows of 3 frequencies for 3 of 2)
    and a count-spectrum group (2 rows of 3 bins for 3 of 4).  The data are made once; returns seven functions that add one group
    each to a fitter.  No new free parameter."""
    truth = tv._c4_truth()
    rng = np.random.default_rng(70)
    bt = tc.EPOCHS[1::8][:2]
    bflux = tc.device_flux([_abi.make_params(**configs.C4_TRUTH)], bt, tl.BAND, 7)[0]
    band = dict(band=tl.BAND, t=bt, flux=bflux * (1 + 0.05 * rng.standard_normal(2)), err=0.1 * bflux, num_points=7)
    ct = np.array([100.0, 300.0]) * DAY
    sm = truth.sky_moments(ct, 5e9, exact=True)
    err = np.full(2, 0.2 * tv.units.mas)
    cen = dict(nu=5e9, t=ct, east=tv.EAST0_TRUE + sm.Xbar * np.sin(tv.PA_TRUE) + sm.Ybar * np.cos(tv.PA_TRUE) + 0.5 * err,
               north=sm.Xbar * np.cos(tv.PA_TRUE) - sm.Ybar * np.sin(tv.PA_TRUE) - 0.5 * err, err_east=err, err_north=1.5 * err)
    vd = tv.make_group(truth, tv.VIS_T[:2], tv.VIS_NU, (3, 2), tv.PA_TRUE, tv.EAST0_TRUE, seed=2)
    pol = tp.make_group(truth, t=tp.POL_T[:3], seed=2)
    counts = tc.make_group(tc.EPOCHS[5::6][:2], np.full(2, 5e4), 1, seed=12)
    index = ti.make_group(ti.X_BAND, tc.EPOCHS[2::5][:4], 3, "slope", seed=34)
    fold = tf.make_group(3, 2, tc.EPOCHS[5::7][:2], np.full(2, 4e4), 1, seed=52, absorption=True,
                         truth=np.append(tc.TRUTH, tf.LOG_N_H_TRUE), d=tf.defs(tf.N_H_DEF))
    return [lambda f: f.add_flux(**band), lambda f: f.add_centroid(**cen), lambda f: tv.add_group(f, vd, n_az=64),
            lambda f: tp.add_group(f, pol), lambda f: f.add_counts(**counts), lambda f: f.add_spectral_index(**index),
            lambda f: f.add_count_spectrum(**fold)]


def fixture_d():
    """Nine fitters on fixture (c)'s data: F0 = fixture (c); F_1 .. F_7 = F0 plus one of the extra_groups() each; F_all = F0 plus all
    seven, so that every list kind has two groups of different row counts (the correlated groups are two already).  Returns
    ([F0, F_1, ..., F_7, F_all], parameter list): the parameters are fixture (c)'s."""
    base, d = fixture_c()
    fits = [copy.deepcopy(base) for _ in range(9)]  # (before any of them has built a spec)
    for k, add in enumerate(extra_groups()):
        add(fits[1 + k])
        add(fits[8])
    return fits, d


def n_passes(spec):
    """The passes of a likelihood call on this spec: the point rows, then one per group of every list."""
    lists = (spec._sky, spec._vis, spec._pol, spec._counts, spec._index, spec._fold, spec._cov)
    return (1 if spec.n_data > 0 else 0) + spec.n_bands + sum(s.n_groups for s in lists if s is not None)


def walkers_a(nb):
    return np.ascontiguousarray(tv._walkers(nb, seed=12)[0])


def walkers_b(nb):
    th, sky = tv._walkers(nb, seed=12)
    rng = np.random.default_rng(21)
    return np.ascontiguousarray(np.column_stack([th, sky, rng.uniform(0.2, 0.8, nb), rng.uniform(0.0, 0.2, nb)]))


def walkers_c(nb):
    rng = np.random.default_rng(33)
    return np.ascontiguousarray(np.column_stack([walkers_b(nb), rng.uniform(0.1, 0.6, nb), rng.uniform(21.5, 22.5, nb)]))


@pytest.fixture(scope="module")
def fit_a():
    return fixture_a()


@pytest.fixture(scope="module")
def fit_b():
    return fixture_b()


@pytest.fixture(scope="module")
def fit_c():
    return fixture_c()


ENTRY_POINTS = ("", "sky_", "vis_", "pol_", "lim_", "noise_", "counts_", "index_")  # entry point k takes the first k optional specs


def call(name, spec, optional, samples, dev=False):
    """One entry point by name on the shared context: `optional` are its spec arguments after the fit spec (ctypes structs or None).
    dev: the device-pointer form, its arguments torch tensors on the GPU.  Returns ln L as a numpy array."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    ref = [C.byref(x) if x is not None else None for x in optional]
    nb = samples.shape[0]
    if not dev:
        out = np.empty(nb)
        with lock:
            _lib.check(getattr(lib, name)(h, C.byref(spec), *ref, samples.ctypes.data_as(dp), nb, spec.ndim, out.ctypes.data_as(dp)))
        return out
    import torch
    theta = torch.from_numpy(samples).to("cuda:0")
    out = torch.empty((nb,), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with lock:
        _lib.check(getattr(lib, name + "_dev")(h, C.byref(spec), *ref, theta.data_ptr(), nb, spec.ndim, out.data_ptr()))
        _lib.check(lib.vag_ctx_synchronize(h))
    return out.cpu().numpy()


def all_specs(spec):
    return [spec._sky, spec._vis, spec._pol, spec._lim, spec._noise, spec._counts, spec._index]


def widest_specs(spec):
    return all_specs(spec) + [spec._fold, spec._tmpl, spec._cov]


@pytest.mark.parametrize("nb", BATCHES)
def test_point_data_through_all_sixteen_entry_points(fit_a, nb):
    """Fixture (a) through every entry point, host and device-pointer form: with the optional specs NULL, and with them present
    and empty (n_groups = 0; the limit and noise specs cover every row and flag none).  The bits of vag_loglike_batch every time."""
    f, d = fit_a
    spec, _, _ = f.build_spec(d)
    assert all(s is None for s in all_specs(spec)) and spec.n_data == 60 and spec.n_bands == 0
    th = walkers_a(nb)
    base = call("vag_loglike_batch", spec, [], th)
    assert np.all(np.isfinite(base))
    kind = np.zeros(60, dtype=np.int32)  # all detections; limit / sigma stay NULL: they are not read
    lim = _lib.LimitFitSpec()
    lim.point.kind = kind.ctypes.data_as(ip)
    group = np.full(60, -1, dtype=np.int32)  # no row in a group
    noise = _lib.NoiseFitSpec()
    noise.point_group = group.ctypes.data_as(ip)
    empty = [_lib.SkyFitSpec(), _lib.VisFitSpec(), _lib.PolFitSpec(), lim, noise, _lib.CountsFitSpec(), _lib.IndexFitSpec()]
    for k, name in enumerate(ENTRY_POINTS):
        for optional in ([None] * k, empty[:k]):
            for dev in (False, True):
                got = call(f"vag_loglike_{name}batch", spec, optional, th, dev=dev)
                assert np.array_equal(got, base), (name, dev, optional[:1])


@pytest.mark.parametrize("nb", BATCHES)
def test_every_kind_of_data_in_one_fit(fit_b, nb):
    """Fixture (b): the host form equals the device-pointer form, a repeat call (at 64 walkers: in the evaluation order the first
    call left) and a call under VAG_NO_ORDER are equal, and Fitter.loglike_batch is vag_loglike_index_batch -- all to the bits."""
    f, d = fit_b
    spec, _, _ = f.build_spec(d)
    assert all(s is not None for s in all_specs(spec))
    assert (spec.n_data, spec.n_bands, spec._sky.n_groups, spec._vis.n_groups, spec._pol.n_groups) == (12, 1, 1, 1, 1)
    assert (spec._counts.n_groups, spec._index.n_groups, spec._noise.n_groups) == (1, 1, 1)
    th = walkers_b(nb)
    a = call("vag_loglike_index_batch", spec, all_specs(spec), th)
    assert np.all(np.isfinite(a))
    assert np.array_equal(call("vag_loglike_index_batch", spec, all_specs(spec), th, dev=True), a)
    assert np.array_equal(call("vag_loglike_index_batch", spec, all_specs(spec), th), a)
    assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: call("vag_loglike_index_batch", spec, all_specs(spec), th)), a)
    assert np.array_equal(f.loglike_batch(th, d), a)
    assert f.last_plan.n_walkers_rejected == 0


def test_the_resident_centroid_visibility_and_polarization_blocks_follow_the_data(fit_b):
    """Two fitters of fixture (b)'s shapes whose centroid, visibility and polarization groups hold other values, called A, A, B, A,
    B on the shared context at 3 walkers: a block of the same size and another content is uploaded anew each time the data change,
    so every A is the first A, every B the first B, and A is not B -- all to the bits."""
    (fa, d), (fb, _) = fit_b, fixture_b(other=True)
    sa, sb = fa.build_spec(d)[0], fb.build_spec(d)[0]
    assert (sa._sky.groups[0].n, sa._vis.groups[0].n_vis, sa._pol.groups[0].n) == (sb._sky.groups[0].n, sb._vis.groups[0].n_vis, sb._pol.groups[0].n)
    th = walkers_b(3)
    a1, a2, b1, a3, b2 = (call("vag_loglike_index_batch", s, all_specs(s), th) for s in (sa, sa, sb, sa, sb))
    assert np.all(np.isfinite(a1)) and np.all(np.isfinite(b1))
    assert np.array_equal(a2, a1) and np.array_equal(a3, a1)
    assert np.array_equal(b2, b1)
    assert np.all(a1 != b1)


@pytest.mark.parametrize("nb", BATCHES)
def test_every_kind_of_data_through_the_widest_entry_point(fit_c, nb):
    """Fixture (c), what fixture (b) gets: the host form equals the device-pointer form, a repeat call and a call under VAG_NO_ORDER
    are equal, and Fitter.loglike_batch is vag_loglike_cov_batch -- all to the bits."""
    f, d = fit_c
    spec, _, _ = f.build_spec(d)
    assert all(s is not None for s in widest_specs(spec))
    assert (spec.n_data, spec.n_bands, spec._fold.n_groups, spec._tmpl.n_templates, spec._cov.n_groups) == (15, 1, 1, 1, 2)
    assert sorted(spec._cov.groups[g].n for g in range(2)) == [2, 65] and bool(spec._fold.groups[0].sigma)
    th = walkers_c(nb)
    a = call("vag_loglike_cov_batch", spec, widest_specs(spec), th)
    assert np.all(np.isfinite(a))
    assert np.array_equal(call("vag_loglike_cov_batch", spec, widest_specs(spec), th, dev=True), a)
    assert np.array_equal(call("vag_loglike_cov_batch", spec, widest_specs(spec), th), a)
    assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: call("vag_loglike_cov_batch", spec, widest_specs(spec), th)), a)
    assert np.array_equal(f.loglike_batch(th, d), a)
    assert f.last_plan.n_walkers_rejected == 0


def test_a_second_group_of_every_kind_adds_its_own_term():
    """Fixture (d) at 3 walkers (the identity evaluation order).  With one group per kind every group starts at offset 0 of its
    resident block and the call's last pass is the only one of its kind: a pass that read a column of the wrong group, or a wrong
    first or last pass, could not show.  Two groups of different row counts is the smallest shape at which it can.  A pass adds one
    chi^2 term per walker, so ln L(F_all) - ln L(F0) = sum_k (ln L(F_k) - ln L(F0)), exactly in real arithmetic; on the device each
    side adds one term per pass in double, so the two sides agree within N 2^-52 max |ln L|, N the passes of the nine fits that
    enter, counted from their specs.  Every value is finite and every extra group moves every walker.

    Largest observed ratio of the residual to that bound on an MI355X: 0.0031 (a residual of 2.9e-11, half an ulp of the largest
    |ln L| = 4.0e5, in one walker, against 9.3e-9 for N = 104; the other two walkers exact), in this build and in its parent alike."""
    fits, d = fixture_d()
    th = walkers_c(3)
    specs = [f.build_spec(d)[0] for f in fits]
    assert [n_passes(s) for s in specs] == [10] + [11] * 7 + [17]

    def groups(s):
        return (s.n_bands, s._sky.n_groups, s._vis.n_groups, s._pol.n_groups, s._counts.n_groups, s._index.n_groups, s._fold.n_groups)

    assert groups(specs[0]) == (1,) * 7 and groups(specs[8]) == (2,) * 7 and specs[8]._cov.n_groups == 2
    ll = np.array([f.loglike_batch(th, d) for f in fits])  # [9][3]
    assert np.all(np.isfinite(ll))
    assert np.all(ll[1:8] != ll[0])
    residual = np.abs((ll[8] - ll[0]) - np.sum(ll[1:8] - ll[0], axis=0))
    bound = sum(n_passes(s) for s in specs) * 2.0 ** -52 * np.max(np.abs(ll))
    print(f"residual {residual.tolist()} bound {bound!r} ratio {np.max(residual) / bound!r} max |ln L| {np.max(np.abs(ll))!r}")
    assert np.all(residual <= bound)


@pytest.mark.parametrize("nb", BATCHES)
def test_an_out_of_range_walker_of_every_kind_of_data(fit_c, nb):
    """The same as the next test on fixture (c), under the same pin and for the same reason."""
    f, d = fit_c
    th = walkers_c(nb)
    bad = th.copy()
    bad[1, 0] = -0.05

    def both():
        base = f.loglike_batch(th, d)
        return base, f.loglike_batch(bad, d), f.last_plan.n_walkers_rejected

    base, out, rejected = tv._with_hook("VAG_PAIRS_PER_BLOCK", "4", both)
    assert np.all(np.isfinite(base))
    assert out[1] == -np.inf and np.array_equal(np.delete(out, 1), np.delete(base, 1))
    assert rejected == 1


@pytest.mark.parametrize("nb", BATCHES)
def test_an_out_of_range_walker_scores_minus_infinity(fit_b, nb):
    """theta_c < 0 in one walker of fixture (b): the walker is -inf, the others keep their bits, the plan counts one rejection.

    Both calls run with the (theta, phi) pairs per flux workgroup pinned (the VAG_PAIRS_PER_BLOCK hook, at 4: the floor of the
    engine's own choice).  A band request takes that number from the batch's total work (choose_pairs_per_block), the rejected
    walker's lattice leaves the total, and the partial sums of the other walkers' band fluxes are then cut elsewhere -- the batch
    dependence of a band group's last bits that loglike_body describes where it pins the number for a counts pass.  It is the flux
    request's, not the closing block's: unpinned, one walker of the 64 (walker 16) moves by 1 ulp of ln L, in this build and in
    the build before the back kernels shared their closing block alike; at 3 walkers none moves."""
    f, d = fit_b
    th = walkers_b(nb)
    bad = th.copy()
    bad[1, 0] = -0.05

    def both():
        base = f.loglike_batch(th, d)
        return base, f.loglike_batch(bad, d), f.last_plan.n_walkers_rejected

    base, out, rejected = tv._with_hook("VAG_PAIRS_PER_BLOCK", "4", both)
    assert np.all(np.isfinite(base))
    assert out[1] == -np.inf and np.array_equal(np.delete(out, 1), np.delete(base, 1))
    assert rejected == 1


@pytest.mark.parametrize("nb", BATCHES)
def test_an_out_of_range_walker_of_the_point_data(fit_a, nb):
    """The same on fixture (a), nothing pinned: a series request does not take its partial sums from the batch."""
    f, d = fit_a
    th = walkers_a(nb)
    base = f.loglike_batch(th, d)
    assert np.all(np.isfinite(base))
    bad = th.copy()
    bad[1, 0] = -0.05
    out = f.loglike_batch(bad, d)
    assert out[1] == -np.inf and np.array_equal(np.delete(out, 1), np.delete(base, 1))
    assert f.last_plan.n_walkers_rejected == 1
