"""What the model requests refuse, in which words and in which order: the fourteen host-pointer entry points and the two
device-pointer ones (vag_flux_density_grid_batch_dev, vag_flux_density_batch_dev).  Per entry the order is: its own null-pointer
checks that come before the context (the out4 forms), a null context, its own null / empty / range checks, what check_host_inputs
refuses (null model or time, empty batch, empty, bad or descending times, "model %d: ..."), and only then the split of a batch of
mixed flags and the device -- the batch here is A B A (plain, reverse shock, plain), and an invalid third model is reported as
"model 2", its place in the caller's batch, not in its group.  The band entries' own refusals (band_request_dev) come behind the
uploads.  Every return code and text is a literal copied from vag_capi.hip; for each two neighbours of an entry's list a call with
both faults must give the first one's text.  The calls need a context and reach no kernel, but for the two good requests that end
the null-frequency test."""
import ctypes as C
import types

import numpy as np
import pytest

import _abi
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
INVALID, HIP_ERROR, CAPACITY = -1, -3, -5  # VAG_E_INVALID, VAG_E_HIP, VAG_E_CAPACITY (include/vegasafterglow_amd.h)
NAN = float("nan")
KEEP = []  # the arrays behind the pointers


def ptr(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    KEEP.append(a)
    return a.ctypes.data_as(dp)


def models(bad_third=False):
    rvs = dict(eps_e=0.1, eps_B=0.01, p=2.3)
    kws = [dict(theta_obs=0.1), dict(theta_obs=0.1, duration=50.0, rvs=rvs), dict(theta_obs=0.2)]
    prms = [_abi.make_params(**kw) for kw in kws]
    if bad_third:
        prms[2].eps_e = 0.0
    arr = (_lib.ModelParams * 3)(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in prms])
    KEEP.append(arr)
    return arr


def pol_specs(b=(1.0, 1.0, 1.0), pi_max1=(-1.0, -1.0, -1.0)):
    arr = (_lib.PolSpec * 3)()
    for m in range(3):
        arr[m].b[0], arr[m].b[1] = b[m], 1.0
        arr[m].pi_max[0], arr[m].pi_max[1] = -1.0, pi_max1[m]
    KEEP.append(arr)
    return arr


@pytest.fixture(scope="module")
def eng():
    import torch  # (the device-pointer entries' arguments are real device arrays: a refusal that failed to come would not run wild)
    lib = _lib.load()
    h, _ = va.get_context(0)
    dev = torch.device("cuda:0")
    d = types.SimpleNamespace(params=torch.frombuffer(bytearray(bytes(models())), dtype=torch.uint8).to(dev),
                              t=torch.tensor([1e4, 1e5, 1e6], dtype=torch.float64, device=dev),
                              nu=torch.tensor([1e9, 1e15, 1e17], dtype=torch.float64, device=dev),
                              out=torch.zeros(64, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    return lib, h, d


def good(h, d):
    """Arguments every entry accepts: three models of two flag sets, nt = 3, nnu = 2, npixel = 8, n_az = 32, nbl = 4, a band of 5."""
    out = [ptr(np.zeros(1 << 14)) for _ in range(5)]
    return dict(c=h, params=models(), nb=3, t=ptr([1e4, 1e5, 1e6]), nt=3, nu=ptr([1e9, 1e15, 1e17]), nnu=2, out=out[0], out2=out[1],
                out4=(dp * 4)(*out[1:5]), fov=1e-3, npixel=8, n_az=32, u=ptr(np.full(24, 1e6)), v=ptr(np.full(24, 2e6)), nbl=4, pa=0.3,
                pol=pol_specs(), nu_min=1e14, nu_max=1e15, num_nu=5, d_params=C.c_void_p(d.params.data_ptr()),
                d_t=C.c_void_p(d.t.data_ptr()), d_nu=C.c_void_p(d.nu.data_ptr()), d_out=C.c_void_p(d.out.data_ptr()))


CALLS = {
    "vag_flux_density_grid_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.out),
    "vag_flux_density_grid_components_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.out, a.out2),
    "vag_flux_density_grid_components4_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.out4),
    "vag_sky_image_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.fov, a.npixel, a.n_az, a.out, a.out2),
    "vag_sky_moments_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.n_az, a.out),
    "vag_sky_centroid_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.out),
    "vag_sky_visibility_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.u, a.v, a.nbl, a.pa, a.n_az, a.out),
    "vag_sky_polarization_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.pol, a.pa, a.n_az, a.out),
    "vag_sky_stokes_image_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu, a.nnu, a.pol, a.fov, a.npixel, a.n_az, a.out, a.out2),
    "vag_flux_density_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nu, a.nt, a.out),
    "vag_flux_density_components4_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nu, a.nt, a.out4),
    "vag_flux_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu_min, a.nu_max, a.num_nu, a.out),
    "vag_flux_components_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu_min, a.nu_max, a.num_nu, a.out, a.out2),
    "vag_flux_components4_batch": lambda L, a: L(a.c, a.params, a.nb, a.t, a.nt, a.nu_min, a.nu_max, a.num_nu, a.out4),
    "vag_flux_density_grid_batch_dev": lambda L, a: L(a.c, a.d_params, a.nb, a.d_t, a.nt, a.d_nu, a.nnu, a.d_out),
    "vag_flux_density_batch_dev": lambda L, a: L(a.c, a.d_params, a.nb, a.d_t, a.d_nu, a.nt, a.d_out),
}

CTX = [(dict(c=None), "null context")]
NNU = [(dict(nnu=0), "frequency array must be non-empty"), (dict(nnu=-1), "frequency array must be non-empty")]
FOV = [(dict(fov=0.0), "fov must be positive and finite"), (dict(fov=float("inf")), "fov must be positive and finite"),
       (dict(npixel=0), "npixel must be in [1, 4096]"), (dict(npixel=4097), "npixel must be in [1, 4096]")]
BAND = [(dict(nu_min=0.0), "nu_min must be positive"), (dict(nu_max=1e14), "nu_max must be greater than nu_min"),
        (dict(num_nu=1), "num_nu must be at least 2"), (dict(num_nu=65), "at most 64 band frequencies", CAPACITY)]


def nulls(keys, text):
    return [({k: None}, text) for k in keys]


def host_inputs(time_first=False):
    """check_host_inputs, in its order.  time_first: the null time before the null model (the same refusal)."""
    null = [(dict(params=None), "null model or time array"), (dict(t=None), "null model or time array")]
    return (null[::-1] if time_first else null) + [
        (dict(nb=0), "batch must be non-empty"), (dict(nt=0), "time array must be non-empty"),
        (dict(t=ptr([1e4, -1.0, 1e6])), "times must be positive and finite"), (dict(t=ptr([1e4, NAN, 1e6])), "times must be positive and finite"),
        (dict(t=ptr([1e4, 1e6, 1e5])), "time array must be in ascending order"),
        (dict(params=models(bad_third=True)), "model 2: eps_e must be in (0, 1]")]


def pol_refusals():
    return [(dict(pol=pol_specs(b=(1.0, -1.0, 1.0))), "model 1: pol.b[0] must be finite and >= 0"),
            (dict(pol=pol_specs(b=(1.0, NAN, 1.0))), "model 1: pol.b[0] must be finite and >= 0"),
            (dict(pol=pol_specs(pi_max1=(1.5, -1.0, -1.0))), "model 0: pol.pi_max[1] must be <= 1 (< 0: from p)")]


def refusals(name):
    """The entry's refusals in the order in which it makes them: (what is wrong, the text[, the code])."""
    if name == "vag_flux_density_grid_batch":
        return CTX + nulls(["nu", "out"], "null frequency or output array") + NNU + host_inputs()
    if name == "vag_flux_density_grid_components_batch":
        return CTX + NNU + host_inputs()
    if name == "vag_flux_density_grid_components4_batch":
        return nulls(["out4"], "out4 must not be null") + nulls(["nu"], "null frequency array") + CTX + NNU + host_inputs()
    if name == "vag_sky_image_batch":
        return CTX + nulls(["nu", "out"], "null frequency or image array") + NNU + FOV + host_inputs()
    if name in ("vag_sky_moments_batch", "vag_sky_centroid_batch"):
        return CTX + nulls(["nu", "out"], "null frequency or moments array") + NNU + host_inputs()
    if name == "vag_sky_visibility_batch":
        return (CTX + nulls(["nu", "u", "v", "out"], "null frequency, baseline or visibility array") + NNU +
                [(dict(nbl=0), "nbl must be in [1, 65536], got 0"), (dict(nbl=65537), "nbl must be in [1, 65536], got 65537"),
                 (dict(u=ptr([1e6] * 23 + [NAN])), "baselines u, v must be finite"), (dict(v=ptr([float("inf")] + [1e6] * 23)), "baselines u, v must be finite"),
                 (dict(pa=NAN), "pa must be finite")] + host_inputs())
    if name == "vag_sky_polarization_batch":  # (the spec is read per model: not where there is no model, see the extra cases)
        return (CTX + nulls(["nu", "pol", "out"], "null frequency, polarization spec or output array") + NNU + [(dict(pa=NAN), "pa must be finite")] +
                pol_refusals() + host_inputs(time_first=True))
    if name == "vag_sky_stokes_image_batch":
        return (CTX + nulls(["nu", "pol", "out"], "null frequency, polarization spec or image array") + NNU + FOV + pol_refusals() +
                host_inputs(time_first=True))
    if name == "vag_flux_density_batch":
        return CTX + nulls(["nu", "out"], "null frequency or output array") + host_inputs()
    if name == "vag_flux_density_components4_batch":
        return CTX + nulls(["out4"], "out4 must not be null") + nulls(["nu"], "null frequency array") + host_inputs()
    if name == "vag_flux_batch":
        return CTX + nulls(["out"], "null output array") + host_inputs() + BAND
    if name == "vag_flux_components_batch":
        return CTX + host_inputs() + BAND
    if name == "vag_flux_components4_batch":
        return nulls(["out4"], "out4 must not be null") + CTX + host_inputs() + BAND
    if name == "vag_flux_density_grid_batch_dev":
        return (CTX + nulls(["d_params", "d_t", "d_nu", "d_out"], "null device pointer") +
                [({k: 0}, "empty batch, time or frequency array") for k in ("nb", "nt", "nnu")])
    if name == "vag_flux_density_batch_dev":
        return (CTX + nulls(["d_params", "d_t", "d_nu", "d_out"], "null device pointer") +
                [({k: 0}, "empty batch or data array") for k in ("nb", "nt")])
    raise KeyError(name)


def refused(eng, name, wrong, text, code=INVALID):
    lib, h, d = eng
    a = good(h, d)
    a.update(wrong)
    rc = CALLS[name](getattr(lib, name), types.SimpleNamespace(**a))
    assert (rc, lib.vag_last_error().decode()) == (code, text), (name, sorted(wrong))


@pytest.mark.parametrize("name", list(CALLS))
def test_every_refusal_keeps_its_code_its_words_and_its_place(eng, name):
    cases = refusals(name)
    for wrong, text, *code in cases:
        refused(eng, name, wrong, text, *code)
    for (w0, text, *code), (w1, *_) in zip(cases, cases[1:]):  # two faults at once: the earlier refusal wins
        if not set(w0) & set(w1):
            refused(eng, name, {**w0, **w1}, text, *code)


def test_a_null_frequency_array_the_entry_does_not_check_is_refused_by_the_upload(eng):
    """vag_flux_density_grid_components_batch has no null check of nu: the upload of d_nu refuses the null source (VAG_E_HIP, the text
    names the call, the runtime's words and a source line), behind check_host_inputs and ahead of any kernel; the context then serves
    requests as before (the first one may still meet the runtime's remembered error; the second may not)."""
    lib, h, d = eng
    name = "vag_flux_density_grid_components_batch"
    for wrong in (dict(nu=None), dict(nu=None, out=None, out2=None)):
        a = good(h, d)
        a.update(wrong)
        rc = CALLS[name](getattr(lib, name), types.SimpleNamespace(**a))
        text = lib.vag_last_error().decode()
        assert rc == HIP_ERROR and text.startswith("hipMemcpyAsync(c->d_nu.p, ") and " failed: " in text, (rc, text)
    refused(eng, name, dict(nu=None, nt=0), "time array must be non-empty")
    a = types.SimpleNamespace(**good(h, d))
    CALLS[name](getattr(lib, name), a)
    assert CALLS[name](getattr(lib, name), a) == 0, lib.vag_last_error().decode()


def test_what_is_not_looked_at(eng):
    """The baselines are read only where there is a time to read them for; the polarization spec only where there are models."""
    refused(eng, "vag_sky_visibility_batch", dict(nt=0, u=ptr([NAN] * 24)), "time array must be non-empty")
    refused(eng, "vag_sky_visibility_batch", dict(nt=0, u=ptr([NAN] * 24), pa=NAN), "pa must be finite")
    bad = pol_specs(b=(-1.0, 1.0, 1.0))
    for name in ("vag_sky_polarization_batch", "vag_sky_stokes_image_batch"):
        refused(eng, name, dict(params=None, pol=bad), "null model or time array")
        refused(eng, name, dict(nb=0, pol=bad), "batch must be non-empty")
        refused(eng, name, dict(nt=0, pol=bad), "model 0: pol.b[0] must be finite and >= 0")
