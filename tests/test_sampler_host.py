"""The device sampler's host side (no GPU): the counter-based draws, the numpy statement of the move, the refusals.

1. sampling.philox4x32 reproduces the three Random123 known-answer vectors of Philox4x32-10;
2. csrc/vag_philox.h -- the text the kernels compile -- does the same in tests/philox_check.cpp, a stand-alone program built with the
   system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer as tests/test_fit_request_host.py builds its program, and run as
   a child process: the vectors, the ends of u53, the partner index, the ends of stretch_z (below a even where the
   fma rounds t up to a; sampling.stretch_z keeps the same half-open end).  Nothing is loaded into this process;
3. the host statement (run_stretch_move_philox: fixed halves, Philox draws, fused proposals) samples a 3-D Gaussian, and no decision
   of that run is closer to its threshold than 1e-9 -- the condition under which tests/test_sampler.py compares the device's decisions
   exactly;
4. the Python-side refusals;
5. thinning and continuing a run (step0) do not change a bit of run_stretch_move_philox's chain."""
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

import test_fit_request_host as host  # FLAGS, STATIC: the sanitizer build of the other stand-alone program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = [  # Random123 kat_vectors, philox4x32 10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
MU, SIGMA = np.array([0.5, -2.0, 30.0]), np.array([1.0, 0.1, 10.0])
GAUSS_SEED = 3  # (the issue's seed: it passes the margin condition with the fused proposals, min |margin| = 3.1e-5)


def gaussian_log_prob(x):
    return -0.5 * np.sum(((np.asarray(x) - MU) / SIGMA) ** 2, axis=1)


def gaussian_start(nwalkers=32):
    return MU + SIGMA * np.random.default_rng(0).standard_normal((nwalkers, 3))


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert [int(v) for v in sampling.philox4x32(counter, key)] == list(want)
    # vectorised: the three vectors in one call, and a key broadcast over counters
    out = sampling.philox4x32(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert out.dtype == np.uint32 and out.tolist() == [list(k[2]) for k in KAT]
    two = sampling.philox4x32(np.zeros((2, 4), dtype=np.uint32), [0, 0])
    assert two.shape == (2, 4) and two[1].tolist() == list(KAT[0][2])


# ---- 2. the header under the host sanitizers ----

PHILOX_CASES = ["vector zeros", "vector ones", "vector pi", "vector in place", "u53 zero", "u53 top", "partner top", "partner zero",
                "stretch_z low", "stretch_z high"]
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)


@pytest.fixture(scope="module")
def philox_lines(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("philox") / "philox_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "philox_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    lines = ran.stdout.splitlines()
    assert ran.returncode == sum(ln.startswith("FAIL") for ln in lines), ran.stdout  # (its exit status counts its failures)
    return lines


@pytest.mark.parametrize("case", PHILOX_CASES)
def test_philox_header_under_asan_and_ubsan(philox_lines, case):
    assert f"ok {case}" in philox_lines, philox_lines


def test_stretch_factor_stays_below_a_in_numpy_too():
    """stretch_z(2, 1 - 2^-53) < 2 ("stretch_z high" above): t = fma(1, 1 - 2^-53, 1) ties to 2 and t t / a would be a itself, so
    the header keeps the half-open end -- the largest double below a -- and sampling.stretch_proposals must do the same to stay its
    statement to the bit.  Here: the numpy side at the ends of [0, 1) and over the last uniforms below 1, for both scales the
    device test uses."""
    top = 1.0 - 2.0 ** -53 * np.arange(1, 9)
    assert sampling.stretch_z(2.0, 0.0) == 0.5 and sampling.stretch_z(2.0, top[0]) == np.nextafter(2.0, 0.0)
    for a in (2.0, 1.5):
        z = sampling.stretch_z(a, top)
        assert np.all(z < a) and np.all(z >= sampling.stretch_z(a, 0.5)) and np.all(np.diff(z) <= 0)
        assert sampling.stretch_z(a, 0.0) == 1 / a
    pos = np.random.default_rng(0).standard_normal((64, 2))
    for a in (2.0, 1.5):
        z = np.concatenate([sampling.stretch_proposals(pos, s, h, 0, a)[1] for s in range(50) for h in (0, 1)])
        assert np.all((z >= 1 / a) & (z < a))


# ---- 3. the host statement samples a Gaussian ----

@pytest.fixture(scope="module")
def gaussian_run():
    margins = []
    chain, logp, acc = sampling.run_stretch_move_philox(gaussian_log_prob, gaussian_start(), 2000, seed=GAUSS_SEED, margins=margins)
    return chain, logp, acc, np.concatenate(margins)


def test_host_statement_samples_a_gaussian(gaussian_run):
    chain, logp, acc, margins = gaussian_run
    assert chain.shape == (2000, 32, 3) and logp.shape == (2000, 32) and margins.shape == (2000 * 32,)
    x = (chain[200:].reshape(-1, 3) - MU) / SIGMA
    mean, var = x.mean(axis=0), x.var(axis=0)
    print("standardised mean", mean, "variance", var, "acceptance", acc.mean(), "min |margin|", np.abs(margins).min())
    assert np.all(np.abs(mean) < 0.15), mean
    assert np.all((var > 0.88) & (var < 1.12)), var  # (without z^(ndim-1): 0.51; with z^ndim or a uniform z: 1.26-1.30)
    assert 0.55 < acc.mean() < 0.75, acc.mean()
    assert np.array_equal(logp[-1], gaussian_log_prob(chain[-1]))  # positions and stored ln p belong together
    # no decision sits on its threshold: the device (another log, another rounding of the sum) decides every one the same way
    assert np.abs(margins).min() > 1e-9


def test_proposals_and_decisions():
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((10, 3))
    for half in (0, 1):
        prop, z, partner = sampling.stretch_proposals(pos, 7, half, 11, 2.0)
        mine = np.arange(half * 5, half * 5 + 5)
        assert prop.shape == (5, 3) and np.all((z >= 0.5) & (z <= 2.0))
        assert np.all((partner >= (1 - half) * 5) & (partner < (2 - half) * 5))  # always of the other half
        np.testing.assert_allclose(prop, pos[partner] + z[:, None] * (pos[mine] - pos[partner]), rtol=1e-14, atol=1e-15)
        # the draws depend on (seed, step, walker) alone
        again = sampling.stretch_proposals(pos, 7, half, 11, 2.0)
        assert all(np.array_equal(u, v) for u, v in zip((prop, z, partner), again))
        assert not np.array_equal(z, sampling.stretch_proposals(pos, 8, half, 11, 2.0)[1])
        assert not np.array_equal(z, sampling.stretch_proposals(pos, 7, half, 12, 2.0)[1])
    z = np.full(5, 1.0)
    lp_new = np.array([0.0, np.nan, np.inf, -np.inf, 50.0])
    take, margin = sampling.stretch_accepts(0, 0, 0, z, lp_new, np.zeros(5), 3)
    assert take.tolist() == [bool(margin[0] > 0), False, False, False, True]  # not finite: rejected, NaN and +inf too
    assert np.all(margin[1:4] == -np.inf)


# ---- 4. refusals on the Python side (before any device is looked for) ----

def test_python_side_refusals():
    lp = lambda x: np.zeros(len(x))  # noqa: E731
    with pytest.raises(ValueError, match="even number of walkers"):
        sampling.run_stretch_move_philox(lp, np.zeros((7, 2)), 1)
    with pytest.raises(ValueError, match="even number of walkers"):
        sampling.run_stretch_move_philox(lp, np.zeros((4, 3)), 1)
    with pytest.raises(ValueError, match="a must be finite and > 1"):
        sampling.run_stretch_move_philox(lp, np.zeros((4, 2)), 1, a=1.0)
    with pytest.raises(ValueError, match="thin must be >= 1"):
        sampling.run_stretch_move_philox(lp, np.zeros((4, 2)), 1, thin=0)
    with pytest.raises(ValueError, match="initial positions must have finite log-probability"):
        sampling.run_stretch_move_philox(lambda x: np.full(len(x), -np.inf), np.zeros((4, 2)), 1)
    with pytest.raises(ValueError, match="even number of walkers"):
        sampling.StretchMove(7, 2)
    with pytest.raises(ValueError, match="even number of walkers"):
        sampling.StretchMove(4, 3)
    with pytest.raises(ValueError, match="a must be finite and > 1"):
        sampling.StretchMove(4, 2, a=0.5)
    with pytest.raises(ValueError, match="a must be finite and > 1"):
        sampling.StretchMove(4, 2, a=float("nan"))
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    for bad in (dict(pos0=np.zeros((5, 2))), dict(pos0=np.zeros((2, 2))), dict(pos0=np.zeros((4, 2)), a=1.0),
                dict(pos0=np.zeros((4, 2)), thin=0)):
        with pytest.raises(ValueError):
            sampling.run_stretch_move_device(fitter, defs, nsteps=1, **bad)
    with pytest.raises(ValueError, match="loglike_fn"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="device", loglike_fn=lambda s: np.zeros(len(s)))
    with pytest.raises(ValueError, match="unknown sampler"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="gpu")
    with pytest.raises(ValueError, match="unknown sampler"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="gpu")


# ---- 5. thinning and continuing ----

def test_thin_and_chunks_do_not_change_the_chain():
    pos0 = gaussian_start(8)
    chain, logp, acc = sampling.run_stretch_move_philox(gaussian_log_prob, pos0, 30, seed=2 ** 40 + 7)
    thin_chain, thin_logp, thin_acc = sampling.run_stretch_move_philox(gaussian_log_prob, pos0, 30, seed=2 ** 40 + 7, thin=3)
    assert thin_chain.shape == (10, 8, 3)
    assert np.array_equal(thin_chain, chain[2::3]) and np.array_equal(thin_logp, logp[2::3]) and np.array_equal(thin_acc, acc)
    # a run continued from where another stopped is the one run: steps are absolute
    first = sampling.run_stretch_move_philox(gaussian_log_prob, pos0, 11, seed=2 ** 40 + 7)
    rest = sampling.run_stretch_move_philox(gaussian_log_prob, first[0][-1], 19, seed=2 ** 40 + 7, step0=11)
    assert np.array_equal(np.concatenate([first[0], rest[0]]), chain) and np.array_equal(np.concatenate([first[1], rest[1]]), logp)
    assert np.allclose(first[2] * 11 + rest[2] * 19, acc * 30)
    # ... thinned too: the stored steps are the same absolute ones ((s + 1) % 3 == 0)
    rest3 = sampling.run_stretch_move_philox(gaussian_log_prob, first[0][-1], 19, seed=2 ** 40 + 7, step0=11, thin=3)
    assert np.array_equal(rest3[0], chain[11:][0::3]) and rest3[0].shape[0] == 7
