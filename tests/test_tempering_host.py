"""Parallel tempering's host side (no GPU): the margins of the header, the numpy statement of the move, the evidence, the refusals.

1. csrc/vag_tempering.h -- the text the kernels compile -- forms its two margins in tests/tempering_check.cpp, a stand-alone program
   built under AddressSanitizer + UndefinedBehaviorSanitizer as tests/test_sampler_host.py builds philox_check.cpp and run as a child
   process; sampling.tempered_log_ratio / swap_log_ratio give the same bits over its table (beta = 0 and 1, equal ln L, huge
   differences, rows where the fma and the unfused form differ).  Nothing is loaded into this process;
2. a bimodal target (two Gaussians 40 sigma apart, weights 0.7 / 0.3) started in one mode: the tempered cold chain visits the
   other mode with its weight, the plain move (one rung) never does; no decision sits on its threshold;
3. the evidence of a Gaussian likelihood under a uniform prior: the mean ln L per rung against quadrature, thermodynamic_evidence
   against the trapezoid rule on the exact means, and that rule's known gap to the true ln Z;
4. continuing (step0) and thinning do not change a bit; one rung is run_stretch_move_philox;
5. the Python-side refusals."""
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

import test_fit_request_host as host  # FLAGS, STATIC: the sanitizer build of the other stand-alone programs
import test_sampler_host as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)

BOX = 6.0
LN_PRIOR = -np.log((2 * BOX) ** 2)  # uniform on [-6, 6]^2


def box_log_prior(x):
    return np.where(np.all(np.abs(np.asarray(x)) <= BOX, axis=1), LN_PRIOR, -np.inf)


def bimodal_log_like(x):
    """ln of 0.7 N((-2, 0), 0.1^2) + 0.3 N((2, 0), 0.1^2)"""
    x = np.asarray(x)
    a = np.log(0.7) - 0.5 * ((x[:, 0] + 2.0) ** 2 + x[:, 1] ** 2) / 0.01
    b = np.log(0.3) - 0.5 * ((x[:, 0] - 2.0) ** 2 + x[:, 1] ** 2) / 0.01
    return np.logaddexp(a, b) - np.log(2 * np.pi * 0.01)


def bimodal_start(ntemps, nw, seed):
    return np.array([-2.0, 0.0]) + 0.05 * np.random.default_rng(seed).standard_normal((ntemps, nw, 2))


def all_margins(margins):
    return np.concatenate([m.ravel() for m in margins])


# ---- 1. the header under the host sanitizers ----

@pytest.fixture(scope="module")
def header_rows(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("tempering") / "tempering_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "tempering_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    assert ran.returncode == 0, ran.stdout
    rows = {"ratio": [], "swap": []}
    for ln in ran.stdout.splitlines():
        kind, *words = ln.split()
        rows[kind].append(np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64))
    return {k: np.array(v) for k, v in rows.items()}


def test_header_margins_are_the_numpy_margins_to_the_bit(header_rows):
    r, s = header_rows["ratio"], header_rows["swap"]
    assert r.shape[1] == 6 and s.shape[1] == 5 and len(r) >= 8 and len(s) >= 5
    want = sampling.tempered_log_ratio(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4])
    assert np.array_equal(want.view(np.uint64), r[:, 5].view(np.uint64)), (want, r[:, 5])
    want_s = sampling.swap_log_ratio(s[:, 0], s[:, 1], s[:, 2], s[:, 3])
    assert np.array_equal(want_s.view(np.uint64), s[:, 4].view(np.uint64)), (want_s, s[:, 4])
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(s))
    # what the table holds: both ends of the ladder, equal ln L, huge differences, and rows that tell the fma from a product and a sum
    unfused = r[:, 0] * (r[:, 1] - r[:, 2]) + (r[:, 3] - r[:, 4])
    assert np.any(r[:, 0] == 0) and np.any(r[:, 0] == 1) and np.any(r[:, 1] == r[:, 2]) and np.any(np.abs(r[:, 1] - r[:, 2]) > 1e29)
    # (the two differ by the rounding of the product, at most half an ulp of it, and each by half an ulp of its own sum)
    assert np.sum(unfused != r[:, 5]) >= 2
    assert np.all(np.abs(unfused - r[:, 5]) <= 2.0 ** -52 * (np.abs(r[:, 0] * (r[:, 1] - r[:, 2])) + np.abs(r[:, 5])))
    assert np.all(r[r[:, 0] == 0, 5] == r[r[:, 0] == 0, 3] - r[r[:, 0] == 0, 4])  # beta = 0: the priors alone
    plain = (r[:, 0] == 1) & (r[:, 3] == r[:, 4])
    assert np.any(plain) and np.all(r[plain, 5] == r[plain, 1] - r[plain, 2])  # beta = 1, equal priors: the plain move's difference
    assert np.any(s[:, 1] == 0) and np.any(s[:, 0] == 1) and np.any(np.abs(s[:, 4]) > 1e29)
    assert np.any(s[:, 2] == s[:, 3]) and np.all(s[s[:, 2] == s[:, 3], 4] == 0)  # equal ln L: log(u) < 0 always exchanges


# ---- 2. the bimodal target ----

@pytest.fixture(scope="module", params=[1, 2, 3])
def bimodal_run(request):
    seed = request.param
    betas = sampling.geometric_betas(6, 1e-3)
    pos0 = bimodal_start(6, 32, seed)
    margins = []
    out = sampling.run_tempered_philox(bimodal_log_like, box_log_prior, pos0, betas, 1500, seed=seed, margins=margins)
    return seed, pos0, out, margins


def test_tempering_finds_the_second_mode_and_the_plain_move_does_not(bimodal_run):
    seed, pos0, (chain, lnl, lnprior, acc, swap_fraction), margins = bimodal_run
    assert chain.shape == (1500, 6, 32, 2) and lnl.shape == lnprior.shape == (1500, 6, 32)
    assert acc.shape == (6, 32) and swap_fraction.shape == (5,) and len(margins) == 1500 * 3
    fraction = (chain[750:, 0, :, 0] > 0).mean()
    smallest = np.abs(all_margins(margins)).min()
    print("seed", seed, "cold fraction in the second mode", fraction, "cold acceptance", acc[0].mean(), "swap fractions", swap_fraction,
          "min |margin|", smallest)
    assert 0.2 <= fraction <= 0.4, fraction
    assert smallest > 1e-9
    assert 0.2 < acc[0].mean() < 0.8, acc[0].mean()
    assert np.all((swap_fraction > 0.1) & (swap_fraction < 0.9)), swap_fraction
    assert np.all(np.isfinite(lnl)) and np.all(lnprior == LN_PRIOR)  # every state is inside the box
    assert np.array_equal(lnl[-1].ravel(), bimodal_log_like(chain[-1].reshape(-1, 2)))  # positions and stored ln L belong together
    # the same start at one temperature: the plain stretch move never leaves the mode it started in
    one_margins = []
    one = sampling.run_tempered_philox(bimodal_log_like, box_log_prior, pos0[:1], [1.0], 1500, seed=seed, margins=one_margins)
    assert (one[0][750:, 0, :, 0] > 0).mean() == 0.0 and one[4].shape == (0,)
    assert np.abs(all_margins(one_margins)).min() > 1e-9


# ---- 3. the evidence ----

SIGMA = 0.5
LN_Z_TRUE = -2.0 * np.log(2 * BOX)  # the normalised Gaussian lies well inside the box: Z = 1 / 144


def gaussian_log_like(x):
    return -np.log(2 * np.pi * SIGMA ** 2) - 0.5 * np.sum(np.asarray(x) ** 2, axis=1) / SIGMA ** 2


def exact_mean_log_like(beta):
    """<ln L> under L^beta times the uniform prior: each coordinate is a Gaussian of variance sigma^2 / beta truncated to the box;
    <x^2> by Gauss-Legendre quadrature, 200 nodes on each of 60 panels."""
    x, w = np.polynomial.legendre.leggauss(200)
    edges = np.linspace(-BOX, BOX, 61)
    xx = (0.5 * (edges[1:] - edges[:-1])[:, None] * x + 0.5 * (edges[1:] + edges[:-1])[:, None]).ravel()
    ww = (0.5 * (edges[1:] - edges[:-1])[:, None] * w).ravel()
    f = ww * np.exp(-0.5 * beta * xx ** 2 / SIGMA ** 2)
    return -np.log(2 * np.pi * SIGMA ** 2) - 2.0 * (np.sum(f * xx ** 2) / np.sum(f)) / (2 * SIGMA ** 2)


@pytest.fixture(scope="module")
def evidence_ladder():
    betas = sampling.geometric_betas(8, 1e-2, prior_rung=True)
    exact = np.array([exact_mean_log_like(b) for b in betas])
    return betas, exact


def test_the_rule_on_the_exact_means_and_its_known_gap(evidence_ladder):
    betas, exact = evidence_ladder
    assert exact[0] == pytest.approx(-np.log(2 * np.pi * SIGMA ** 2) - 1.0, abs=1e-9)  # beta = 1: <r^2> = 2 sigma^2
    assert exact[-1] == pytest.approx(-np.log(2 * np.pi * SIGMA ** 2) - 2 * 12.0 / (2 * SIGMA ** 2), abs=1e-9)  # the prior: <x^2> = 12
    ln_z, err = sampling.thermodynamic_evidence(betas, exact)
    assert ln_z == pytest.approx(-5.273, abs=1e-3)
    # the discretisation error of this ladder's rule: <ln L> is steep towards beta = 0 and the trapezoids overshoot by 0.30;
    # the estimate from every second rung (0.99) is above it here
    assert ln_z - LN_Z_TRUE == pytest.approx(-0.303, abs=2e-3) and abs(ln_z - LN_Z_TRUE) < err
    # a finer ladder closes the gap
    fine = np.append(np.geomspace(1.0, 1e-4, 63), 0.0)
    ln_z_fine, err_fine = sampling.thermodynamic_evidence(fine, np.array([exact_mean_log_like(b) for b in fine]))
    assert abs(ln_z_fine - LN_Z_TRUE) < 0.02 and err_fine < 0.1


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_thermodynamic_evidence_of_a_gaussian(evidence_ladder, seed):
    betas, exact = evidence_ladder
    pos0 = 0.3 * np.random.default_rng(seed).standard_normal((8, 32, 2))
    chain, lnl, lnprior, acc, swap_fraction = sampling.run_tempered_philox(gaussian_log_like, box_log_prior, pos0, betas, 2000, seed=seed)
    mean = lnl[500:].mean(axis=(0, 2))
    ln_z, err = sampling.thermodynamic_evidence(betas, mean)
    want, _ = sampling.thermodynamic_evidence(betas, exact)
    print("seed", seed, "max relative error of <ln L>", np.abs(mean / exact - 1).max(), "ln Z", ln_z, "+-", err, "rule on exact means", want)
    assert np.all(np.abs(mean / exact - 1) < 0.03), mean / exact
    assert abs(ln_z - want) < 0.1, (ln_z, want)
    assert np.all(np.abs(chain) <= BOX)  # the prior rung too stays inside the box


def test_thermodynamic_evidence_by_hand():
    ln_z, err = sampling.thermodynamic_evidence([1.0, 0.5, 0.0], [-1.0, -2.0, -6.0])
    assert ln_z == pytest.approx(0.5 * -1.5 + 0.5 * -4.0) and err == pytest.approx(abs(ln_z - -3.5))
    ln_z, err = sampling.thermodynamic_evidence([1.0, 0.5, 0.25, 0.0], [-1.0, -2.0, -3.0, -6.0])  # an even ladder keeps its last rung
    assert ln_z == pytest.approx(0.5 * -1.5 + 0.25 * -2.5 + 0.25 * -4.5) and err == pytest.approx(abs(ln_z - (0.75 * -2.0 + 0.25 * -4.5)))
    assert sampling.thermodynamic_evidence([1.0], [-3.0]) == (0.0, 0.0)
    with pytest.raises(ValueError):
        sampling.thermodynamic_evidence([1.0, 0.0], [-1.0])


# ---- 4. continuing, thinning, one rung ----

def test_continuation_and_thinning_do_not_change_a_bit():
    betas = sampling.geometric_betas(3, 1e-2)
    pos0 = bimodal_start(3, 8, 5)
    seed = 2 ** 40 + 7
    run = lambda *a, **kw: sampling.run_tempered_philox(bimodal_log_like, box_log_prior, *a, seed=seed, **kw)  # noqa: E731
    full = run(pos0, betas, 30)
    thin = run(pos0, betas, 30, thin=3)
    assert thin[0].shape == (10, 3, 8, 2)
    assert all(np.array_equal(t, f[2::3]) for t, f in zip(thin[:3], full[:3])) and np.array_equal(thin[3], full[3])
    assert np.array_equal(thin[4], full[4])
    first = run(pos0, betas, 11)
    rest = run(first[0][-1], betas, 19, step0=11)
    assert all(np.array_equal(np.concatenate([a, b]), f) for a, b, f in zip(first[:3], rest[:3], full[:3]))
    assert np.allclose(first[3] * 11 + rest[3] * 19, full[3] * 30)
    # the attempts follow from the parity rule: pair t is tried at the steps s with t + s even
    assert sampling.swap_attempts(3, 0, 11).tolist() == [6, 5] and sampling.swap_attempts(3, 11, 19).tolist() == [9, 10]
    attempts = sampling.swap_attempts(3, 0, 30) * 8
    assert np.allclose(first[4] * sampling.swap_attempts(3, 0, 11) * 8 + rest[4] * sampling.swap_attempts(3, 11, 19) * 8, full[4] * attempts)
    rest3 = run(first[0][-1], betas, 19, step0=11, thin=3)
    assert np.array_equal(rest3[0], full[0][11:][0::3]) and rest3[0].shape[0] == 7


def test_one_rung_is_the_plain_move():
    pos0 = sh.gaussian_start()
    chain, logp, acc = sampling.run_stretch_move_philox(sh.gaussian_log_prob, pos0, 200, seed=sh.GAUSS_SEED)
    one = sampling.run_tempered_philox(sh.gaussian_log_prob, lambda x: np.zeros(len(x)), pos0[None], [1.0], 200, seed=sh.GAUSS_SEED)
    assert np.array_equal(one[0][:, 0], chain) and np.array_equal(one[1][:, 0], logp) and np.all(one[2] == 0)
    assert np.array_equal(one[3][0], acc) and one[4].shape == (0,)


def test_building_blocks():
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((3, 10, 2))
    for half in (0, 1):
        prop, z, partner = sampling.tempered_proposals(pos, 7, half, 11)
        assert prop.shape == (3, 5, 2) and np.all((partner >= (1 - half) * 5) & (partner < (2 - half) * 5))
        for t in range(3):  # every temperature stretches within its own ensemble
            np.testing.assert_allclose(prop[t], pos[t][partner[t]] + z[t][:, None] * (pos[t][half * 5:half * 5 + 5] - pos[t][partner[t]]),
                                       rtol=1e-14, atol=1e-15)
        # the cold rung draws what the plain move draws: r = w there
        plain = sampling.stretch_proposals(pos[0], 7, half, 11)
        assert np.array_equal(prop[0], plain[0]) and np.array_equal(z[0], plain[1]) and np.array_equal(partner[0], plain[2])
        assert not np.array_equal(z[1], z[0]) and not np.array_equal(z[2], z[1])
    # not finite: rejected at every temperature, beta = 0 included
    z = np.ones((2, 4))
    bad = np.array([np.nan, np.inf, -np.inf, 1e300])
    zero = np.zeros((2, 4))
    for betas in ([1.0, 0.5], [1.0, 0.0]):
        take, margin = sampling.tempered_accepts(0, 0, 0, z, betas, np.tile(bad, (2, 1)), zero, zero, zero, 2)
        assert take[0].tolist() == [False, False, False, True] and np.all(margin[:, :3] == -np.inf)
        assert take[1].tolist() == [False, False, False, betas[1] > 0 or bool(margin[1, 3] > 0)]
        take, margin = sampling.tempered_accepts(0, 0, 0, z, betas, zero, np.tile(bad, (2, 1)), zero, zero, 2)
        assert np.all(take[:, :3] == False) and np.all(take[:, 3]) and np.all(margin[:, :3] == -np.inf)  # noqa: E712
    # exchanges: the pairs of the step's parity, and a hot walker with the higher ln L always moves down
    lnl = np.array([[-5.0, -1.0], [-1.0, -5.0], [-2.0, -2.0], [0.0, -9.0]])
    lower, take, margin = sampling.tempered_swaps(4, 0, [1.0, 0.5, 0.25, 0.0], lnl)
    assert lower.tolist() == [0, 2] and take.shape == (2, 2) and take[0, 0] and take[1, 0]
    lower, take, margin = sampling.tempered_swaps(5, 0, [1.0, 0.5, 0.25, 0.0], lnl)
    assert lower.tolist() == [1] and take.shape == (1, 2)
    assert sampling.tempered_swaps(5, 0, [1.0, 0.5], lnl[:2])[0].size == 0


# ---- 5. refusals on the Python side (before any device is looked for) ----

def test_python_side_refusals():
    ll, lp = (lambda x: np.zeros(len(x))), (lambda x: np.zeros(len(x)))
    run = lambda pos0, betas, **kw: sampling.run_tempered_philox(ll, lp, pos0, betas, 1, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="start at 1"):
        run(np.zeros((2, 4, 2)), [0.9, 0.5])
    with pytest.raises(ValueError, match="strictly descending"):
        run(np.zeros((3, 4, 2)), [1.0, 0.5, 0.5])
    with pytest.raises(ValueError, match="strictly descending"):
        run(np.zeros((3, 4, 2)), [1.0, 0.2, 0.5])
    with pytest.raises(ValueError, match=">= 0"):
        run(np.zeros((2, 4, 2)), [1.0, -0.1])
    with pytest.raises(ValueError, match="finite"):
        run(np.zeros((2, 4, 2)), [1.0, np.nan])
    with pytest.raises(ValueError, match="1..64"):
        run(np.zeros((65, 4, 2)), np.linspace(1.0, 0.0, 65))
    with pytest.raises(ValueError, match="one ensemble per entry"):
        run(np.zeros((3, 4, 2)), [1.0, 0.5])
    with pytest.raises(ValueError, match="even number of walkers"):
        run(np.zeros((2, 7, 2)), [1.0, 0.5])
    with pytest.raises(ValueError, match="even number of walkers"):
        run(np.zeros((2, 4, 3)), [1.0, 0.5])
    with pytest.raises(ValueError, match="1..16 dimensions"):
        run(np.zeros((2, 40, 17)), [1.0, 0.5])
    with pytest.raises(ValueError, match="thin must be >= 1"):
        run(np.zeros((2, 4, 2)), [1.0, 0.5], thin=0)
    with pytest.raises(ValueError, match="finite ln L and ln prior"):
        sampling.run_tempered_philox(ll, lambda x: np.full(len(x), -np.inf), np.zeros((2, 4, 2)), [1.0, 0.5], 1)
    for bad in (dict(betas=[0.9, 0.5], nwalkers=4, ndim=2), dict(betas=[1.0, 1.0], nwalkers=4, ndim=2),
                dict(betas=[1.0, -1.0], nwalkers=4, ndim=2), dict(betas=np.linspace(1.0, 0.0, 65), nwalkers=4, ndim=2),
                dict(betas=[1.0, 0.5], nwalkers=7, ndim=2), dict(betas=[1.0, 0.5], nwalkers=4, ndim=3),
                dict(betas=[1.0, 0.5], nwalkers=40, ndim=17), dict(betas=[1.0, 0.5], nwalkers=4, ndim=2, a=1.0)):
        with pytest.raises(ValueError):
            sampling.TemperedMove(**bad)
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    for bad in (dict(pos0=np.zeros((2, 5, 2)), betas=[1.0, 0.5]), dict(pos0=np.zeros((2, 2, 2)), betas=[1.0, 0.5]),
                dict(pos0=np.zeros((2, 4, 2)), betas=[1.0, 0.5], thin=0), dict(pos0=np.zeros((2, 4, 2)), betas=[0.5, 0.1]),
                dict(pos0=np.zeros((2, 4, 2)), betas=[1.0, 0.5, 0.1]), dict(pos0=np.zeros((4, 2)), betas=[1.0]),
                dict(pos0=np.zeros((2, 4, 2)), betas=[1.0, 0.5], a=1.0)):
        with pytest.raises(ValueError):
            sampling.run_tempered_device(fitter, defs, nsteps=1, **bad)
    with pytest.raises(ValueError, match="loglike_fn"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="tempered", loglike_fn=lambda s: np.zeros(len(s)))
    with pytest.raises(ValueError, match="loglike_fn"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="tempered", loglike_fn=lambda s: np.zeros(len(s)))
    with pytest.raises(ValueError, match="unknown sampler"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="tempering")
    with pytest.raises(ValueError, match="'tempered'"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="gpu")
    with pytest.raises(ValueError, match="ntemps"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="tempered", ntemps=65)


def test_geometric_betas():
    b = sampling.geometric_betas(6, 1e-3)
    assert b.shape == (6,) and b[0] == 1.0 and b[-1] == 1e-3 and np.allclose(b[1:] / b[:-1], 1e-3 ** 0.2)
    assert np.array_equal(b, 1e-3 ** (np.arange(6) / 5.0))
    p = sampling.geometric_betas(8, 1e-2, prior_rung=True)
    assert p.shape == (8,) and p[0] == 1.0 and p[-2] == 1e-2 and p[-1] == 0.0 and np.array_equal(p[:-1], sampling.geometric_betas(7, 1e-2))
    assert sampling.geometric_betas(1).tolist() == [1.0] and sampling.geometric_betas(2, 0.1, prior_rung=True).tolist() == [1.0, 0.0]
    assert sampling.geometric_betas(64).size == 64 and np.all(np.diff(sampling.geometric_betas(64, prior_rung=True)) < 0)
    for bad in (dict(ntemps=0), dict(ntemps=65), dict(ntemps=4, beta_min=0.0), dict(ntemps=4, beta_min=1.0),
                dict(ntemps=4, beta_min=-0.5), dict(ntemps=4, beta_min=float("nan")), dict(ntemps=1, prior_rung=True)):
        with pytest.raises(ValueError):
            sampling.geometric_betas(**bad)
