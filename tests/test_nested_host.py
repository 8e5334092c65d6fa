"""Nested sampling's host side (no GPU): the header's functions, the numpy statement, the evidence, the priors, the refusals.

1. csrc/vag_nested.h -- the text the kernels compile -- forms its rank decisions, live counts and shrinkage terms, ticks, clone
   indices and decision margins in tests/nested_check.cpp, a stand-alone program built under AddressSanitizer +
   UndefinedBehaviorSanitizer as tests/test_tempering_host.py builds tempering_check.cpp and run as a child process; sampling's numpy
   functions give the same bits over its tables.  Nothing is loaded into this process;
2. nested_evidence by hand on N = 4 with two iterations; a continuation (it0) repeats a single run to the bit;
3. the evidence of a 3-D Gaussian likelihood under a uniform prior over eight seeds, against the closed form, with thresholds from
   the theory's standard error sqrt(H_exact / N);
4. the weighted posterior of the same runs;
5. a Gaussian prior narrower than the box: the closed-form evidence against log_prior_mass; sample_prior against the truncated laws;
6. the Python-side refusals, the exported symbols, the ctypes layout against the header, ABI 13."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import _lib, sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale, host_ln_prior

import test_fit_request_host as host  # FLAGS, STATIC: the sanitizer build of the other stand-alone programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- 1. the header under the host sanitizers ----

@pytest.fixture(scope="module")
def header_rows(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("nested") / "nested_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "nested_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    assert ran.returncode == 0, ran.stdout
    rows = {"rank": [], "shrink": [], "tick": [], "clone": [], "margin": []}
    for ln in ran.stdout.splitlines():
        kind, *words = ln.split()
        rows[kind].append([w if w == "|" else int(w, 16) for w in words])
    return rows


def as_double(words):
    return np.array(words, dtype=np.uint64).view(np.float64)


def test_header_rank_decisions_are_numpys(header_rows):
    seen_tie, seen_boundary_tie = False, False
    assert len(header_rows["rank"]) >= 5
    for row in header_rows["rank"]:
        bar = row.index("|")
        lnl, order, lstar = as_double(row[:bar]), np.array(row[bar + 1:-1], dtype=np.int64), as_double(row[-1:])[0]
        n = lnl.size
        want, want_lstar = sampling.nested_order(lnl)
        assert np.array_equal(order, want), (lnl, order, want)
        assert bits(lstar) == bits(want_lstar) and lstar == lnl[order[n // 2 - 1]]
        assert sorted(order.tolist()) == list(range(n))  # a permutation
        ranked = lnl[order]
        assert np.all(np.diff(ranked) >= 0)
        same = np.diff(ranked) == 0
        assert np.all(np.diff(order)[same] > 0)  # equal ln L: ordered by slot
        seen_tie |= bool(same.any())
        seen_boundary_tie |= bool(same[n // 2 - 1])  # the last dead and the first survivor have the same ln L
    assert seen_tie and seen_boundary_tie


def test_header_shrinkage_ticks_and_clones_are_numpys(header_rows):
    s = np.array(header_rows["shrink"], dtype=np.uint64)
    assert len(s) >= 30
    j, n_live, n = s[:, 0].astype(np.int64), s[:, 1].astype(np.int64), s[:, 2].astype(np.int64)
    for jj, nl, nn, term in zip(j, n_live, n, s[:, 3].view(np.float64)):
        assert nn == sampling.nested_live_count(jj, nl) == nl - jj % (nl // 2)
        assert bits(term) == bits(1.0 / float(nn))
        # ... and it is the term nested_evidence sums: ln X after the first point of an iteration at this live count
        if jj % (nl // 2) == 0:
            assert nn == nl
    assert set(n_live.tolist()) == {4, 6, 130, 16384} and n.min() == 3 and n.max() == 16384
    t = np.array(header_rows["tick"], dtype=np.uint64)
    for it, walk, m, tick in t.tolist():
        assert tick == sampling.nested_tick(it, walk, m) == it * (walk + 1) + m
    assert t[:, 3].max() > 2 ** 50 and np.any(t[:, 2] == 0) and np.any(t[:, 2] == t[:, 1])
    for u_bits, k, j0 in header_rows["clone"]:
        u = as_double([u_bits])[0]
        assert j0 == min(int(u * k), k - 1) == math.floor(u * k) and 0 <= j0 < k
    us = as_double([r[0] for r in header_rows["clone"]])
    assert us.min() == 0.0 and us.max() == 1.0 - 2.0 ** -53  # both ends of [0, 1)


def test_header_margins_are_numpys_to_the_bit(header_rows):
    r = as_double(np.array(header_rows["margin"], dtype=np.uint64).ravel()).reshape(-1, 6)
    assert len(r) >= 18
    with np.errstate(all="ignore"):
        want = sampling.nested_margin(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4])
    assert np.array_equal(bits(want), bits(r[:, 5])), (want, r[:, 5])
    take = r[:, 5] > 0
    equal = r[:, 0] == r[:, 3]
    assert equal.sum() >= 2 and not take[equal].any() and np.all(r[equal, 5] == -np.inf)  # ln L' == L*: rejected whatever the draw
    assert np.any(equal & (r[:, 4] == -np.inf))  # ... u = 0 included
    bad = ~np.isfinite(r[:, 0]) | ~np.isfinite(r[:, 1])
    assert bad.sum() >= 7 and np.all(r[bad, 5] == -np.inf) and np.all(r[bad, 4] <= -1.0)  # not finite: rejected whatever the draw
    for col in (0, 1):
        assert np.isnan(r[:, col]).any() and np.any(r[:, col] == np.inf) and np.any(r[:, col] == -np.inf)
    below = (r[:, 0] < r[:, 3]) & np.isfinite(r[:, 0])
    assert below.any() and np.all(r[below, 5] == -np.inf)
    ok = ~bad & (r[:, 0] > r[:, 3])
    assert np.array_equal(bits(r[ok, 5]), bits((r[ok, 1] - r[ok, 2]) - r[ok, 4]))
    assert np.any(r[ok, 5] == 0) and np.any(r[ok, 5] == np.inf) and take[ok].sum() >= 4 and (~take[ok]).sum() >= 2


# ---- 2. the evidence by hand, continuation ----

def test_nested_evidence_by_hand():
    """N = 4, K = 2, two iterations: the live counts are 4, 3, 4, 3."""
    dead = np.array([[-9.0, -7.0], [-5.0, -4.0]])
    live = np.array([-3.0, -2.5, -2.0, -1.0])
    x0 = 1.0
    x1 = math.exp(-1 / 4)
    x2 = math.exp(-1 / 4 - 1 / 3)
    x3 = math.exp(-1 / 4 - 1 / 3 - 1 / 4)
    x4 = math.exp(-1 / 4 - 1 / 3 - 1 / 4 - 1 / 3)
    w = [math.exp(-9.0) * x0 * (1 - math.exp(-1 / 4)), math.exp(-7.0) * x1 * (1 - math.exp(-1 / 3)),
         math.exp(-5.0) * x2 * (1 - math.exp(-1 / 4)), math.exp(-4.0) * x3 * (1 - math.exp(-1 / 3))]
    w += [math.exp(l) * x4 / 4 for l in live]
    # the dead weights are the volumes between successive X (X_{j-1} - X_j), so the eight widths tile [0, 1]
    assert x0 * (1 - math.exp(-1 / 4)) == pytest.approx(x0 - x1) and x3 * (1 - math.exp(-1 / 3)) == pytest.approx(x3 - x4)
    assert (x0 - x1) + (x1 - x2) + (x2 - x3) + (x3 - x4) + 4 * x4 / 4 == pytest.approx(1.0)
    z = sum(w)
    p = np.array(w) / z
    lnl = np.concatenate([dead.ravel(), live])
    h = float(np.sum(p * lnl) - math.log(z))
    ev = sampling.nested_evidence(dead, live)
    assert ev.ln_z == pytest.approx(math.log(z), abs=1e-13) and ev.information == pytest.approx(h, abs=1e-12)
    assert ev.ln_z_err == pytest.approx(math.sqrt(h / 4), abs=1e-12)
    assert ev.log_weights.shape == (8,) and np.allclose(np.exp(ev.log_weights), p, rtol=1e-13, atol=0)
    assert np.array_equal(bits(sampling.nested_evidence(dead.ravel(), live).log_weights), bits(ev.log_weights))
    # the termination measure: what the best live point could still add
    z_dead = sum(w[:4])
    assert sampling.nested_remaining(dead, live) == pytest.approx(math.log((z_dead + math.exp(-1.0) * x4) / z_dead), abs=1e-13)
    assert sampling.nested_remaining(np.empty((0, 2)), live) == math.inf
    # no iteration at all: the live points alone, each 1 / N
    none = sampling.nested_evidence(np.empty((0, 2)), live)
    assert none.ln_z == pytest.approx(math.log(np.mean(np.exp(live))), abs=1e-13)
    with pytest.raises(ValueError):
        sampling.nested_evidence(dead.ravel()[:3], live)
    with pytest.raises(ValueError):
        sampling.nested_evidence(dead, live[:3])
    # systematic resampling: counts within one of n p
    idx = sampling.nested_equal_samples(ev.log_weights, seed=3, n=1000)
    counts = np.bincount(idx, minlength=8)
    assert idx.shape == (1000,) and np.all(np.diff(idx) >= 0) and np.all(np.abs(counts - 1000 * p) < 1.0)
    assert sampling.nested_equal_samples(ev.log_weights, seed=3).shape == (8,)


SIGMA = 0.05


def gauss_log_like(x):
    return -0.5 * np.sum(np.asarray(x) ** 2, axis=1) / SIGMA ** 2 - 3.0 * math.log(SIGMA * math.sqrt(2 * math.pi))


def box_log_prior(x):
    return np.where(np.all(np.abs(np.asarray(x)) <= 1.0, axis=1), -3.0 * math.log(2.0), -np.inf)


def test_continuation_repeats_a_single_run_to_the_bit():
    live0 = np.random.default_rng(4).uniform(-1, 1, (10, 3))
    seed = 2 ** 40 + 7
    m_full, m_parts = [], []
    full = sampling.run_nested_philox(gauss_log_like, box_log_prior, live0, 6, 5, seed=seed, margins=m_full)
    first = sampling.run_nested_philox(gauss_log_like, box_log_prior, live0, 3, 5, seed=seed, margins=m_parts)
    rest = sampling.run_nested_philox(gauss_log_like, box_log_prior, first.live, 3, 5, seed=seed, it0=3, margins=m_parts)
    assert full.niter == 6 and first.niter == rest.niter == 3 and full.ncall == 10 + 6 * 5 * 5
    for name in ("dead_theta", "dead_lnl", "dead_lnprior", "accepted"):
        assert np.array_equal(np.concatenate([getattr(first, name), getattr(rest, name)]), getattr(full, name)), name
    for name in ("live", "lnl", "lnprior"):
        assert np.array_equal(getattr(rest, name), getattr(full, name)), name
    assert len(m_full) == 30 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(m_full, m_parts))
    other = sampling.run_nested_philox(gauss_log_like, box_log_prior, first.live, 3, 5, seed=seed, it0=4)  # another tick: other draws
    assert not np.array_equal(other.live, rest.live)
    # what an iteration is: the dead record is non-decreasing, every live point is above L* of the last iteration, the counts add up
    assert np.all(np.diff(full.dead_lnl.ravel()) >= 0) and np.all(full.lnl >= full.dead_lnl[-1, -1])
    assert np.all((full.accepted >= 0) & (full.accepted <= 25)) and full.accepted.sum() > 0
    assert np.array_equal(full.lnl, gauss_log_like(full.live)) and np.array_equal(full.dead_lnl.ravel(), gauss_log_like(full.dead_theta.reshape(-1, 3)))
    # the building blocks: clones come from the survivors, partners are two distinct survivors
    order, lstar = sampling.nested_order(full.lnl)
    src = sampling.nested_clones(order, 6, 5, seed)
    assert src.shape == (5,) and set(src) <= set(order[5:]) and lstar == full.lnl[order[4]]
    prop, partners, slack = sampling.nested_proposals(full.live, order, 6, 1, 5, seed)
    assert prop.shape == (5, 3) and np.all(partners[:, 0] != partners[:, 1]) and set(partners.ravel()) <= set(order[5:])
    gamma = sampling.de_gamma0(3)
    np.testing.assert_allclose(prop, full.live[order[:5]] + gamma * (full.live[partners[:, 0]] - full.live[partners[:, 1]]), rtol=1e-4)
    # dlogz: niter becomes a maximum, tested at chunk ends; the arrays are those of the plain run of as many iterations
    live256 = np.random.default_rng(0).uniform(-1, 1, (64, 3))
    stopped = sampling.run_nested_philox(gauss_log_like, box_log_prior, live256, 200, 10, seed=1, dlogz=0.5, chunk=3)
    assert 0 < stopped.niter < 200 and stopped.niter % 3 == 0
    plain = sampling.run_nested_philox(gauss_log_like, box_log_prior, live256, stopped.niter, 10, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(stopped, plain))
    assert sampling.nested_remaining(stopped.dead_lnl, stopped.lnl) < 0.5 and stopped.niter > 3
    before = sampling.run_nested_philox(gauss_log_like, box_log_prior, live256, stopped.niter - 3, 10, seed=1)
    assert sampling.nested_remaining(before.dead_lnl, before.lnl) >= 0.5  # the chunk end before did not meet the rule


# ---- 3. and 4. the Gaussian evidence and posterior ----

LN_Z_EXACT = 3.0 * math.log(math.erf(1.0 / (SIGMA * math.sqrt(2.0))) / 2.0)
H_EXACT = -1.5 - 3.0 * math.log(SIGMA * math.sqrt(2 * math.pi)) - LN_Z_EXACT
N_LIVE, WALK, SEEDS = 256, 30, range(8)


def summarise(run):
    ev = sampling.nested_evidence(run.dead_lnl, run.lnl)
    w = np.exp(ev.log_weights)
    samples = np.concatenate([run.dead_theta.reshape(-1, run.live.shape[1]), run.live])
    mean = (w[:, None] * samples).sum(axis=0)
    var = (w[:, None] * (samples - mean) ** 2).sum(axis=0)
    return ev, 1.0 / np.sum(w * w), mean, var


@pytest.fixture(scope="module")
def gaussian_runs():
    out = []
    for seed in SEEDS:
        live0 = np.random.default_rng(seed).uniform(-1, 1, (N_LIVE, 3))
        margins, slacks = [], []
        run = sampling.run_nested_philox(gauss_log_like, box_log_prior, live0, 400, WALK, seed=seed, dlogz=0.01, margins=margins, slacks=slacks)
        out.append((run, margins, slacks) + summarise(run))
    return out


def test_gaussian_evidence_against_the_closed_form(gaussian_runs):
    assert H_EXACT == pytest.approx(6.81, abs=0.005)
    se = math.sqrt(H_EXACT / N_LIVE)
    errors = []
    for seed, (run, margins, slacks, ev, ess, mean, var) in zip(SEEDS, gaussian_runs):
        print("seed", seed, "iterations", run.niter, "ln Z - exact", ev.ln_z - LN_Z_EXACT, "+-", ev.ln_z_err, "H", ev.information, "ESS", ess,
              "acceptance", run.accepted.mean() / (N_LIVE // 2 * WALK))
        assert 0 < run.niter < 400 and run.ncall == N_LIVE + run.niter * (N_LIVE // 2) * WALK
        assert sampling.nested_remaining(run.dead_lnl, run.lnl) < 0.01
        assert abs(ev.ln_z - LN_Z_EXACT) <= 5.0 * se, (seed, ev.ln_z - LN_Z_EXACT)
        assert abs(ev.information / H_EXACT - 1.0) <= 0.10, (seed, ev.information)
        assert abs(ev.ln_z_err / se - 1.0) <= 0.10, (seed, ev.ln_z_err)
        assert np.all(np.diff(run.dead_lnl.ravel()) >= 0) and np.all(np.isfinite(run.dead_lnl))
        # a flat prior: every proposal above L* inside the box is taken, and no decision sits on its threshold
        finite = np.concatenate(margins)
        finite = finite[np.isfinite(finite)]
        assert finite.size and finite.min() > 0 and min(s.min() for s in slacks) > 1e-9
        errors.append(ev.ln_z - LN_Z_EXACT)
    print("mean error", np.mean(errors), "bound", 4.0 * se / math.sqrt(8))
    assert abs(np.mean(errors)) <= 4.0 * se / math.sqrt(8), errors


def test_gaussian_posterior_moments(gaussian_runs):
    """With ESS the Kish size of the weights (measured: 811 .. 880 over the eight seeds, of 2800 stored points), the weighted mean of
    each coordinate lies within 4 sigma / sqrt(ESS) of 0 and the weighted variance within 4 sqrt(2 / ESS) relative of sigma^2."""
    for seed, (run, _, _, ev, ess, mean, var) in zip(SEEDS, gaussian_runs):
        print("seed", seed, "ESS", ess, "mean / (sigma / sqrt ESS)", mean / (SIGMA / math.sqrt(ess)), "(var / sigma^2 - 1) / sqrt(2 / ESS)",
              (var / SIGMA ** 2 - 1) / math.sqrt(2 / ess))
        assert ess > 400
        assert np.all(np.abs(mean) <= 4.0 * SIGMA / math.sqrt(ess)), (seed, mean)
        assert np.all(np.abs(var / SIGMA ** 2 - 1.0) <= 4.0 * math.sqrt(2.0 / ess)), (seed, var)
        assert np.exp(ev.log_weights).sum() == pytest.approx(1.0, abs=1e-12)


# ---- 5. priors ----

PRIOR_S = 0.2  # a Gaussian prior N(0, 0.2^2) per coordinate, narrower than the box [-1, 1]


def gaussian_prior_specs():
    return [(_lib.PRIOR_GAUSSIAN, 0.0, PRIOR_S, None)] * 3


def test_a_gaussian_prior_changes_the_evidence_by_the_analytic_amount():
    """int_box L pi = prod_d N(0; 0, sigma^2 + s^2) (Phi(1 / tau) - Phi(-1 / tau)), tau^2 = sigma^2 s^2 / (sigma^2 + s^2), and the
    run's ln Z is relative to the prior mass inside the box: ln Z = that - log_prior_mass.  H = <ln L>_posterior - ln Z with the
    posterior N(0, tau^2) (its truncation at 20 tau is nothing): <ln L> = -3 ln(sigma sqrt(2 pi)) - 3 tau^2 / (2 sigma^2)."""
    lower, upper, specs = -np.ones(3), np.ones(3), gaussian_prior_specs()
    mass = sampling.prior_mass(lower, upper, specs)
    assert mass == pytest.approx(math.erf(1.0 / (PRIOR_S * math.sqrt(2.0))) ** 3, rel=1e-14)
    tau = SIGMA * PRIOR_S / math.hypot(SIGMA, PRIOR_S)
    per_dim = -0.5 * math.log(2 * math.pi * (SIGMA ** 2 + PRIOR_S ** 2)) + math.log(math.erf(1.0 / (tau * math.sqrt(2.0))))
    ln_z_exact = 3.0 * per_dim - math.log(mass)
    h_exact = -3.0 * math.log(SIGMA * math.sqrt(2 * math.pi)) - 1.5 * tau ** 2 / SIGMA ** 2 - ln_z_exact
    se = math.sqrt(h_exact / N_LIVE)
    flat_shift = ln_z_exact - LN_Z_EXACT  # what the narrower prior adds to the evidence of the flat one
    assert flat_shift == pytest.approx(3.0 * (per_dim - math.log(math.erf(1.0 / (SIGMA * math.sqrt(2.0))) / 2.0)) - math.log(mass))
    log_prior = lambda x: host_ln_prior(x, lower, upper, specs) - math.log(mass)  # noqa: E731 (normalised inside the box)
    errors = []
    for seed in SEEDS:
        live0 = sampling.sample_prior(lower, upper, specs, N_LIVE, np.random.default_rng(seed))
        margins = []
        run = sampling.run_nested_philox(gauss_log_like, log_prior, live0, 400, WALK, seed=seed, dlogz=0.01, margins=margins)
        ev = sampling.nested_evidence(run.dead_lnl, run.lnl)
        print("seed", seed, "iterations", run.niter, "ln Z - exact", ev.ln_z - ln_z_exact, "+-", ev.ln_z_err, "H", ev.information, "exact", h_exact)
        assert abs(ev.ln_z - ln_z_exact) <= 5.0 * se, (seed, ev.ln_z - ln_z_exact)
        assert abs(ev.information / h_exact - 1.0) <= 0.10 and abs(ev.ln_z_err / se - 1.0) <= 0.10
        decided = np.concatenate(margins)
        assert np.abs(decided[np.isfinite(decided)]).min() > 1e-9 and (decided[np.isfinite(decided)] < 0).any()  # the prior does reject
        errors.append(ev.ln_z - ln_z_exact)
    assert abs(np.mean(errors)) <= 4.0 * se / math.sqrt(8), errors
    assert abs(flat_shift) > 5.0 * se  # the two evidences are told apart by the check


def ks_distance(x, cdf):
    x = np.sort(x)
    f = cdf(x)
    n = x.size
    return max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(n) / n))


def test_sample_prior_follows_the_truncated_laws():
    """4096 draws per prior kind against the law truncated to the bounds: the Kolmogorov-Smirnov distance stays within the 0.1 % band
    1.95 / sqrt(4096)."""
    n, band = 4096, 1.95 / math.sqrt(4096)
    lower = np.array([-1.0, 0.5, -0.3, 2.0, 1.0, -1.0])
    upper = np.array([3.0, 2.5, 0.9, 50.0, 8.0, 1.0])
    specs = [(_lib.PRIOR_UNIFORM, 0.0, 0.0, None), (_lib.PRIOR_UNIFORM_RANGE, 1.0, 4.0, None), (_lib.PRIOR_GAUSSIAN, 0.5, 0.4, None),
             (_lib.PRIOR_LOG_UNIFORM, 0.5, 20.0, None), (_lib.PRIOR_GAUSSIAN, -3.0, 1.5, None), (_lib.PRIOR_GAUSSIAN, 0.0, 0.05, None)]
    x = sampling.sample_prior(lower, upper, specs, n, np.random.default_rng(11))
    assert x.shape == (n, 6) and np.all(x >= lower) and np.all(x <= upper)
    assert x[:, 1].min() >= 1.0 and x[:, 3].max() <= 20.0  # a prior's own range cuts the box too
    phi = lambda z: 0.5 * np.vectorize(math.erfc)(-np.asarray(z) / math.sqrt(2.0))  # noqa: E731

    def truncated_normal(mu, s, lo, hi):
        return lambda t: (phi((t - mu) / s) - phi((lo - mu) / s)) / (phi((hi - mu) / s) - phi((lo - mu) / s))
    laws = [lambda t: (t + 1.0) / 4.0, lambda t: (t - 1.0) / 1.5, truncated_normal(0.5, 0.4, -0.3, 0.9),
            lambda t: np.log(t / 2.0) / math.log(10.0), truncated_normal(-3.0, 1.5, 1.0, 8.0),  # (the far tail: 2.7 sigma and beyond)
            truncated_normal(0.0, 0.05, -1.0, 1.0)]
    for d, law in enumerate(laws):
        dist = ks_distance(x[:, d], law)
        print("dimension", d, "KS distance", dist, "band", band)
        assert dist <= band, (d, dist)
    mass = sampling.prior_mass(lower, upper, specs)
    want = 1.0 * (1.5 / 3.0) * float(phi(1.0) - phi(-2.0)) * (math.log(10.0) / math.log(40.0)) * float(phi(11 / 1.5) - phi(4 / 1.5)) * \
        float(phi(20.0) - phi(-20.0))
    assert mass == pytest.approx(want, rel=1e-12)
    assert sampling.prior_mass(lower[:1], upper[:1], specs[:1]) == 1.0
    # the inverse CDF against the CDF, tails included
    p = np.array([1e-300, 1e-20, 1e-5, 0.02425, 0.3, 0.5, 0.7, 0.97575, 1 - 1e-5, 1 - 1e-16])
    assert np.allclose(phi(sampling._norm_ppf(p)), p, rtol=1e-12, atol=0) and sampling._norm_ppf(np.array([0.5]))[0] == 0.0
    for bad_lower, bad_upper, bad_specs in (([5.0], [6.0], [(_lib.PRIOR_UNIFORM_RANGE, 1.0, 4.0, None)]),
                                            ([0.0], [1.0], [(_lib.PRIOR_LOG_UNIFORM, 0.0, 4.0, None)]),
                                            ([0.0], [1.0], [(_lib.PRIOR_GAUSSIAN, 0.0, 0.0, None)]),
                                            ([0.0, 0.0], [1.0, 1.0], [(_lib.PRIOR_UNIFORM, 0.0, 0.0, None)])):
        with pytest.raises(ValueError):
            sampling.sample_prior(np.array(bad_lower), np.array(bad_upper), bad_specs, 4, np.random.default_rng(0))
        with pytest.raises(ValueError):
            sampling.prior_mass(np.array(bad_lower), np.array(bad_upper), bad_specs)


# ---- 6. refusals, symbols, layout ----

class HostOnlyPrior:
    def ln_prob(self, x):
        return np.zeros_like(x)


def test_python_side_refusals():
    ll, lp = (lambda x: np.zeros(len(x))), (lambda x: np.zeros(len(x)))
    run = lambda live0, walk=2, **kw: sampling.run_nested_philox(ll, lp, live0, 1, walk, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="even number of live points"):
        run(np.zeros((7, 2)))
    with pytest.raises(ValueError, match="even number of live points"):
        run(np.zeros((2, 1)))
    with pytest.raises(ValueError, match="4..16384"):
        run(np.zeros((16386, 1)))
    with pytest.raises(ValueError, match="walk"):
        run(np.zeros((4, 2)), walk=0)
    with pytest.raises(ValueError, match="1..16 dimensions"):
        run(np.zeros((40, 17)))
    with pytest.raises(ValueError, match=r"\[n_live, ndim\]"):
        run(np.zeros(4))
    with pytest.raises(ValueError, match="finite ln L and ln prior"):
        sampling.run_nested_philox(lambda x: np.full(len(x), -np.inf), lp, np.zeros((4, 2)), 1, 2)
    with pytest.raises(ValueError, match="finite ln L and ln prior"):
        sampling.run_nested_philox(ll, lambda x: np.full(len(x), np.nan), np.zeros((4, 2)), 1, 2)
    with pytest.raises(ValueError, match="dlogz"):
        run(np.zeros((4, 2)), dlogz=0.0)
    with pytest.raises(ValueError, match="gamma0"):
        run(np.zeros((4, 2)), gamma0=-1.0)
    assert sampling.run_nested_philox(ll, lp, np.zeros((4, 2)), 0, 2).niter == 0
    for bad in (dict(n_live=7, ndim=2, walk=2), dict(n_live=2, ndim=1, walk=2), dict(n_live=16386, ndim=2, walk=2),
                dict(n_live=8, ndim=2, walk=0), dict(n_live=8, ndim=0, walk=2), dict(n_live=40, ndim=17, walk=2),
                dict(n_live=8, ndim=2, walk=2, gamma0=float("nan")), dict(n_live=8, ndim=2, walk=2, sigma=float("inf"))):
        with pytest.raises(ValueError):
            sampling.NestedMove(**bad)
    assert sampling.nested_default_walk(1) == 20 and sampling.nested_default_walk(4) == 20 and sampling.nested_default_walk(16) == 80
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    inside = np.tile([0.1, 52.0], (8, 1))
    for bad in (dict(live0=inside[:7]), dict(live0=inside[:2]), dict(live0=np.tile([0.1, 52.0], (16386, 1))), dict(live0=inside, walk=0),
                dict(live0=inside[:, 0]), dict(live0=np.where(np.arange(16).reshape(8, 2) == 5, np.nan, inside)),
                dict(live0=np.where(np.arange(16).reshape(8, 2) == 2, np.inf, inside)), dict(live0=inside, chunk=0),
                dict(live0=inside, dlogz=-1.0), dict(live0=np.zeros((8, 3)))):
        with pytest.raises(ValueError):
            sampling.run_nested_device(fitter, defs, niter=1, **bad)
    with pytest.raises(ValueError, match="host-only priors"):
        sampling.run_nested_device(fitter, defs, inside, 1, priors={"theta_c": HostOnlyPrior()})
    with pytest.raises(ValueError, match="host-only priors"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", priors={"theta_c": HostOnlyPrior()})
    with pytest.raises(ValueError, match="host-only priors"):
        sampling.sample_prior(np.zeros(1), np.ones(1), [(_lib.PRIOR_NONE, 0.0, 0.0, HostOnlyPrior())], 4, np.random.default_rng(0))
    with pytest.raises(ValueError, match="host-only priors"):
        sampling.prior_mass(np.zeros(1), np.ones(1), [(_lib.PRIOR_NONE, 0.0, 0.0, HostOnlyPrior())])
    with pytest.raises(ValueError, match="loglike_fn"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", loglike_fn=lambda s: np.zeros(len(s)))
    with pytest.raises(ValueError, match="moves"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", moves="reference")
    with pytest.raises(ValueError, match="converge"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", converge=sampling.Convergence())
    with pytest.raises(ValueError, match="even number of live points"):
        fitter.fit(defs, nwalkers=7, nsteps=1, sampler="nested")
    with pytest.raises(ValueError, match="walk"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", walk=0)
    with pytest.raises(ValueError, match="dlogz"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="nested", dlogz=0.0)
    with pytest.raises(ValueError, match="priors"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="device", priors={"theta_c": ("gaussian", 0.1, 0.05)})
    with pytest.raises(ValueError, match="'nested'"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="dynesty")


LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define S(f) offsetof(vag_nested_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_nested_spec), S(seed), S(n_live), S(ndim), S(walk), S(gamma0), S(sigma));
    printf("%d %d\n", VAG_NESTED_MAX_LIVE, VAG_ABI_VERSION);
    return 0;
}
"""


def test_ctypes_layout_matches_header_symbols_are_exported_and_the_abi_stays_13(tmp_path):
    src, exe = tmp_path / "n.c", tmp_path / "n"
    src.write_text(LAYOUT_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    S = _lib.NestedSpec
    assert [int(x) for x in lines[0].split()] == [C.sizeof(S)] + [getattr(S, n).offset for n in ("seed", "n_live", "ndim", "walk", "gamma0", "sigma")]
    assert [int(x) for x in lines[1].split()] == [_lib.NESTED_MAX_LIVE, 13] and _lib.NESTED_MAX_LIVE == sampling.NESTED_MAX_LIVE == 16384
    lib = _lib.load()  # the library the project's build makes for gfx950
    assert len(_lib.NESTED_ENTRIES) == 5
    for name in _lib.NESTED_ENTRIES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert _lib.nested_entry(lib, name) is getattr(lib, name)
    assert lib.vag_abi_version() == 13
