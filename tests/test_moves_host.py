"""The move mix of the device sampler, host side (no GPU): the DE and snooker moves in numpy, the choice of the move, the refusals.

1. csrc/vag_moves.h -- the text the kernels and the C-ABI compile -- in tests/moves_check.cpp, a stand-alone program built with the
   system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer as tests/test_sampler_host.py builds philox_check.cpp, and run
   as a child process: distinct pairs and triples in range at nh = 2, 3, 65 and for the words 0 and 0xffffffff, the choice at the
   weight boundaries, the quantised normal at u1 = 0 and at the largest u1.  Nothing is loaded into this process;
2. the numpy statement agrees with that text where both can be asked the same thing (the choice, the partners);
3. the numpy statement (run_moves_philox) samples the 3-D Gaussian of tests/test_sampler_host.py with DE alone, with snooker alone
   and with the reference mix, within the bounds of that test; snooker alone is the case that catches a wrong Hastings factor
   (variance 0.43-0.49 without it).  No decision of those runs is closer to its threshold than 1e-9 and no DE normal closer to a
   rounding boundary than 1e-9 of a quantum -- the conditions under which tests/test_moves.py compares the device exactly;
4. with the stretch move alone the chain is run_stretch_move_philox's;
5. thin, step0 and continuing a run do not change the chain;
6. the Python-side refusals."""
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

import test_fit_request_host as host
import test_sampler_host as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVES_SEED = 3  # (chosen on the CPU as GAUSS_SEED was: min |margin| 2.5e-5 / 2.0e-4 / 5.3e-5, min slack 2.7e-7 / - / 1.0e-5 for the three mixes)
MIXES = {"de": (("de", 1.0),), "snooker": (("snooker", 1.0),), "reference": sampling.REFERENCE_MOVES}

# ---- 1. the header under the host sanitizers ----

MOVES_CASES = ["pairs nh=2", "pairs nh=3", "pairs nh=65", "triples nh=3", "triples nh=65", "triples cover nh=3", "triples cover nh=65",
               "pair ends", "triple ends", "pair nh=2 top", "choice reference mix", "choice stretch only", "choice no snooker",
               "choice zero first", "choice zero middle", "choice unnormalised", "choice thirds", "choice uniform", "normal u1 zero",
               "normal u1 top", "normal u1 top negative", "quantise ties to even", "gamma0"]
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)


@pytest.fixture(scope="module")
def moves_lines(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("moves") / "moves_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "moves_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    lines = ran.stdout.splitlines()
    assert ran.returncode == sum(ln.startswith("FAIL") for ln in lines), ran.stdout  # (its exit status counts its failures)
    return lines


@pytest.mark.parametrize("case", MOVES_CASES)
def test_moves_header_under_asan_and_ubsan(moves_lines, case):
    assert f"ok {case}" in moves_lines, moves_lines


# ---- 2. numpy and the header say the same ----

def test_numpy_partners_and_choice_are_the_headers():
    """The cases of moves_check.cpp that have a numpy counterpart, with the numbers that program checks."""
    top = np.array([0xFFFFFFFF], dtype=np.uint32)
    zero = np.array([0], dtype=np.uint32)
    assert [int(v[0]) for v in sampling._move_pair(zero, zero, 65)] == [0, 1]
    assert [int(v[0]) for v in sampling._move_pair(top, top, 65)] == [64, 63]
    assert [int(v[0]) for v in sampling._move_pair(top, top, 2)] == [1, 0]
    assert int(sampling._move_triple(zero, zero, zero, 65)[2][0]) == 2 and int(sampling._move_triple(top, top, top, 65)[2][0]) == 62
    words = np.random.default_rng(0).integers(0, 2 ** 32, size=(3, 4000), dtype=np.uint64).astype(np.uint32)
    for nh in (3, 4, 65):
        z, z1, z2 = sampling._move_triple(*words, nh)
        assert np.all((z != z1) & (z != z2) & (z1 != z2))
        assert all(np.all((v >= 0) & (v < nh)) for v in (z, z1, z2))
        if nh < 65:  # (enough draws per pair: the third covers what the first two leave)
            assert set(z2[(z == 0) & (z1 == 1)]) == set(range(2, nh)) and set(z2[(z == nh - 1) & (z1 == 0)]) == set(range(1, nh - 1))
    a, b = sampling._move_pair(words[0], words[1], 2)
    assert np.all(a != b) and set(a) == {0, 1}
    # the choice: a kind of weight 0 is never chosen, the frequencies are the weights
    kinds = np.array([sampling.move_kind(s, 11, (0.0, 0.8, 0.2)) for s in range(4000)])
    assert set(kinds) == {1, 2} and abs((kinds == 1).mean() - 0.8) < 4 * np.sqrt(0.8 * 0.2 / 4000)
    assert {sampling.move_kind(s, 11, (1.0, 0.0, 0.0)) for s in range(200)} == {0}
    assert {sampling.move_kind(s, 11, (0.0, 0.0, 3.0)) for s in range(200)} == {2}
    assert [sampling.move_kind(s, 11, (0.0, 8.0, 2.0)) for s in range(200)] == list(kinds[:200])  # only the ratios matter
    assert sampling.move_kind(2 ** 32 + 5, 2 ** 40 + 7, (1.0, 1.0, 1.0)) in (0, 1, 2)
    assert sampling.de_gamma0(2) == 1.19 and sampling.de_gamma0(8) == 0.595
    n_q, slack = sampling.de_normal(np.array([0.0, 1.0 - 2.0 ** -53]), np.array([0.25, 0.0]))
    assert n_q[0] == 0.0 and abs(n_q[1] - np.sqrt(106.0 * np.log(2.0))) <= 2.0 ** -21 and np.all((slack >= 0) & (slack <= 0.5))
    assert np.array_equal(sampling.move_weights("reference"), [0.0, 0.8, 0.2])


def test_proposals_of_each_kind():
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((12, 3))
    for half in (0, 1):
        mine = np.arange(half * 6, half * 6 + 6)
        prop, factor, partners, slack = sampling.de_proposals(pos, 7, half, 11)
        assert prop.shape == (6, 3) and np.all(factor == 0.0) and np.all(partners // 6 == 1 - half) and np.all(partners[:, 0] != partners[:, 1])
        np.testing.assert_allclose(prop, pos[mine] + sampling.de_gamma0(3) * (pos[partners[:, 0]] - pos[partners[:, 1]]), rtol=1e-3, atol=1e-3)
        assert np.all(np.abs(prop - pos[mine] - sampling.de_gamma0(3) * (pos[partners[:, 0]] - pos[partners[:, 1]])) > 0)  # the jitter is there
        wide = sampling.de_proposals(pos, 7, half, 11, gamma0=2.0, sigma=0.0)[0]
        np.testing.assert_allclose(wide, pos[mine] + 2.0 * (pos[partners[:, 0]] - pos[partners[:, 1]]), rtol=1e-14, atol=1e-15)
        prop, factor, partners = sampling.snooker_proposals(pos, 7, half, 11)
        z, z1, z2 = (pos[partners[:, k]] for k in range(3))
        assert np.all(partners // 6 == 1 - half) and all(len(set(row)) == 3 for row in partners.tolist())
        delta = pos[mine] - z
        unit = delta / np.linalg.norm(delta, axis=1)[:, None]  # the projection on the unit vector of the paper
        want = pos[mine] + 1.7 * np.sum(unit * (z1 - z2), axis=1)[:, None] * unit
        np.testing.assert_allclose(prop, want, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(factor, np.log(np.linalg.norm(prop - z, axis=1) / np.linalg.norm(delta, axis=1)) * 2.0, rtol=1e-12, atol=1e-14)
        # the proposal stays on the line through the walker and z
        assert np.all(np.abs(np.cross(prop - z, delta)) < 1e-12 * (1 + np.abs(prop).max()))
        again = sampling.snooker_proposals(pos, 7, half, 11)
        assert all(np.array_equal(u, v) for u, v in zip((prop, factor, partners), again))
        assert not np.array_equal(partners, sampling.snooker_proposals(pos, 8, half, 11)[2])
    # a walker on its z: r2 = 0, its own position and factor -inf, rejected whatever ln p
    _, _, partners = sampling.snooker_proposals(pos, 7, 0, 11)
    stuck = pos.copy()
    stuck[2] = stuck[partners[2, 0]]
    prop, factor, _ = sampling.snooker_proposals(stuck, 7, 0, 11)
    assert np.array_equal(prop[2], stuck[2]) and factor[2] == -np.inf and np.all(np.isfinite(np.delete(factor, 2)))
    take, margin = sampling.move_accepts(7, 0, 11, factor, np.full(6, 1e300), np.zeros(6))
    assert not take[2] and margin[2] == -np.inf and np.all(np.delete(take, 2))
    # one dimension: the factor is 0 and the step is gamma_s (z1 - z2)
    line = rng.standard_normal((8, 1))
    prop, factor, partners = sampling.snooker_proposals(line, 3, 1, 5)
    assert np.all(factor == 0.0)
    np.testing.assert_allclose(prop, line[4:] + 1.7 * (line[partners[:, 1]] - line[partners[:, 2]]), rtol=1e-13, atol=1e-14)
    lp_new = np.array([0.0, np.nan, np.inf, -np.inf, 50.0])
    take, margin = sampling.move_accepts(0, 0, 0, np.zeros(5), lp_new, np.zeros(5))
    want, _ = sampling.stretch_accepts(0, 0, 0, np.ones(5), lp_new, np.zeros(5), 3)
    assert take.tolist() == want.tolist() == [bool(margin[0] > 0), False, False, False, True] and np.all(margin[1:4] == -np.inf)


# ---- 3. the host statement samples a Gaussian ----

@pytest.fixture(scope="module", params=list(MIXES))
def gaussian_run(request):
    margins, slacks = [], []
    chain, logp, acc = sampling.run_moves_philox(sh.gaussian_log_prob, sh.gaussian_start(), 2000, moves=MIXES[request.param],
                                                 seed=MOVES_SEED, margins=margins, slacks=slacks)
    return request.param, chain, logp, acc, np.concatenate(margins), (np.concatenate(slacks) if slacks else np.empty(0))


def test_host_statement_samples_a_gaussian(gaussian_run):
    name, chain, logp, acc, margins, slacks = gaussian_run
    assert chain.shape == (2000, 32, 3) and logp.shape == (2000, 32) and margins.shape == (2000 * 32,)
    n_de = sum(sampling.move_kind(s, MOVES_SEED, sampling.move_weights(MIXES[name])) == 1 for s in range(2000))
    assert slacks.shape == (n_de * 32,) and n_de == {"de": 2000, "snooker": 0}.get(name, n_de) and (name != "reference" or 1500 < n_de < 1700)
    x = (chain[200:].reshape(-1, 3) - sh.MU) / sh.SIGMA
    mean, var = x.mean(axis=0), x.var(axis=0)
    print(name, "standardised mean", mean, "variance", var, "acceptance", acc.mean(), "min |margin|", np.abs(margins).min(),
          "min slack", slacks.min() if slacks.size else None)
    assert np.all(np.abs(mean) < 0.15), mean
    assert np.all((var > 0.88) & (var < 1.12)), var  # (snooker alone without its Hastings factor: 0.43-0.49)
    assert 0.15 < acc.mean() < 0.45, acc.mean()
    assert np.array_equal(logp[-1], sh.gaussian_log_prob(chain[-1]))  # positions and stored ln p belong together
    # no decision sits on its threshold and no normal on a rounding boundary: the device decides and quantises every one the same way
    assert np.abs(margins).min() > 1e-9
    assert slacks.size == 0 or slacks.min() > 1e-9


# ---- 4. the stretch move alone ----

def test_stretch_alone_is_the_stretch_sampler():
    pos0 = sh.gaussian_start()
    want = sampling.run_stretch_move_philox(sh.gaussian_log_prob, pos0, 200, seed=sh.GAUSS_SEED)
    got = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, 200, moves=(("stretch", 1.0),), seed=sh.GAUSS_SEED)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    got = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, 200, moves=(("stretch", 2.0), ("de", 0.0), ("snooker", 0.0)), a=1.5, seed=7)
    want = sampling.run_stretch_move_philox(sh.gaussian_log_prob, pos0, 200, seed=7, a=1.5)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 5. thinning and continuing ----

def test_thin_and_chunks_do_not_change_the_chain():
    pos0, seed, mix = sh.gaussian_start(8), 2 ** 40 + 7, (("stretch", 1.0), ("de", 1.0), ("snooker", 1.0))
    kinds = {sampling.move_kind(s, seed, (1.0, 1.0, 1.0)) for s in range(30)}
    assert kinds == {0, 1, 2}  # every kind takes part
    chain, logp, acc = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, 30, moves=mix, seed=seed)
    thin_chain, thin_logp, thin_acc = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, 30, moves=mix, seed=seed, thin=3)
    assert thin_chain.shape == (10, 8, 3)
    assert np.array_equal(thin_chain, chain[2::3]) and np.array_equal(thin_logp, logp[2::3]) and np.array_equal(thin_acc, acc)
    first = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, 11, moves=mix, seed=seed)
    rest = sampling.run_moves_philox(sh.gaussian_log_prob, first[0][-1], 19, moves=mix, seed=seed, step0=11)
    assert np.array_equal(np.concatenate([first[0], rest[0]]), chain) and np.array_equal(np.concatenate([first[1], rest[1]]), logp)
    assert np.allclose(first[2] * 11 + rest[2] * 19, acc * 30)
    rest3 = sampling.run_moves_philox(sh.gaussian_log_prob, first[0][-1], 19, moves=mix, seed=seed, step0=11, thin=3)
    assert np.array_equal(rest3[0], chain[11:][0::3]) and rest3[0].shape[0] == 7
    # in pieces of 6, 4 and 1 steps
    for piece in (6, 4, 1):
        pos, rows = pos0, []
        for s0 in range(0, 30, piece):
            part = sampling.run_moves_philox(sh.gaussian_log_prob, pos, min(piece, 30 - s0), moves=mix, seed=seed, step0=s0)
            rows.append(part[0])
            pos = part[0][-1]
        assert np.array_equal(np.concatenate(rows), chain), piece


# ---- 6. refusals on the Python side (before any device is looked for) ----

def test_python_side_refusals():
    lp = lambda x: np.zeros(len(x))  # noqa: E731
    run = sampling.run_moves_philox
    for bad, match in [("de", "unknown move mix"), ((("walk", 1.0),), "unknown move"), ((("de", 0.5), ("de", 0.5)), "listed twice"),
                       ((("de", -1.0),), "finite and >= 0"), ((("de", float("nan")),), "finite and >= 0"),
                       ((("de", float("inf")),), "finite and >= 0"), ((("de", 0.0), ("snooker", 0.0)), "not all be zero"), ((), "not all be zero"),
                       (3, "sequence of"), ((("de",),), "sequence of"), ((("de", "much"),), "sequence of")]:
        with pytest.raises(ValueError, match=match):
            sampling.move_weights(bad)
        with pytest.raises(ValueError, match=match):
            run(lp, np.zeros((8, 2)), 1, moves=bad)
        with pytest.raises(ValueError, match=match):
            sampling.EnsembleMoves(8, 2, moves=bad)
    with pytest.raises(ValueError, match="even number of walkers"):
        run(lp, np.zeros((7, 2)), 1)
    with pytest.raises(ValueError, match="even number of walkers"):
        run(lp, np.zeros((4, 3)), 1)
    with pytest.raises(ValueError, match="at least 4 walkers"):
        run(lp, np.zeros((2, 1)), 1, moves=(("de", 1.0),))
    with pytest.raises(ValueError, match="at least 6 walkers"):
        run(lp, np.zeros((4, 2)), 1)  # (the default mix has the snooker move)
    with pytest.raises(ValueError, match="at least 6 walkers"):
        sampling.EnsembleMoves(4, 1, moves=(("stretch", 1.0), ("snooker", 1e-3)))
    sampling.move_weights((("stretch", 1.0), ("snooker", 0.0)))  # (a weight of 0 asks nothing of the ensemble)
    assert sampling._check_moves(np.array([1.0, 0.0, 0.0]), 2, 1) == sampling.de_gamma0(1)
    with pytest.raises(ValueError, match="a must be finite and > 1"):
        run(lp, np.zeros((8, 2)), 1, a=1.0)
    with pytest.raises(ValueError, match="thin must be >= 1"):
        run(lp, np.zeros((8, 2)), 1, thin=0)
    for kw in (dict(gamma0=0.0), dict(gamma0=-1.0), dict(gamma0=float("nan")), dict(gamma0=float("inf")), dict(sigma=float("nan")),
               dict(sigma=float("inf")), dict(gamma_snooker=float("nan")), dict(gamma_snooker=float("-inf"))):
        with pytest.raises(ValueError, match="gamma0 must be finite and > 0|sigma and gamma_snooker must be finite"):
            run(lp, np.zeros((8, 2)), 1, **kw)
        with pytest.raises(ValueError, match="gamma0 must be finite and > 0|sigma and gamma_snooker must be finite"):
            sampling.EnsembleMoves(8, 2, **kw)
    with pytest.raises(ValueError, match="initial positions must have finite log-probability"):
        run(lambda x: np.full(len(x), -np.inf), np.zeros((8, 2)), 1)
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    for bad in (dict(pos0=np.zeros((5, 2))), dict(pos0=np.zeros((2, 2))), dict(pos0=np.zeros((4, 2))), dict(pos0=np.zeros((8, 2)), a=1.0),
                dict(pos0=np.zeros((8, 2)), thin=0), dict(pos0=np.zeros((8, 2)), moves="stretch"), dict(pos0=np.zeros((8, 2)), gamma0=-1.0),
                dict(pos0=np.zeros((8,))), dict(pos0=np.zeros((8, 2)), chunk=0)):
        with pytest.raises(ValueError):
            sampling.run_moves_device(fitter, defs, nsteps=1, **bad)
    for sampler in ("host", "tempered"):
        with pytest.raises(ValueError, match="moves selects the proposals of sampler='device'"):
            sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler=sampler, moves="reference")
        with pytest.raises(ValueError, match="moves selects the proposals of sampler='device'"):
            fitter.fit(defs, nwalkers=8, nsteps=1, sampler=sampler, moves=sampling.REFERENCE_MOVES)
    with pytest.raises(ValueError, match="unknown move mix"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="device", moves="emcee")
    with pytest.raises(ValueError, match="loglike_fn"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="device", moves="reference", loglike_fn=lambda s: np.zeros(len(s)))
