"""Parallel tempering on the device (vag_loglike_split_dev, vag_tempered_propose_dev / _accept_dev / _swap_dev / _run_dev;
sampling.TemperedMove, run_tempered_device, Fitter.log_like_and_prior_batch, fit(sampler="tempered")) against its numpy statement
(sampling.tempered_proposals, tempered_accepts, tempered_swaps, run_tempered_philox).  Results are compared with np.array_equal:
the proposals and the two margins are fused operations and exact differences, and the decisions of the runs compared here are all
further than 1e-9 from their thresholds (asserted), far above the rounding of a logarithm.

1. proposal bits over ladders, sizes, halves, steps and seeds beyond 2^32 and two scales;
2. decisions, exchanges and chain bits on the bimodal problem of tests/test_tempering_host.py, ln L and ln prior formed on the host;
3. a proposal whose ln L or ln prior is not finite is rejected at every temperature, beta = 0 included;
4. vag_loglike_split_dev / Fitter.log_like_and_prior_batch against log_prob_batch and loglike_batch;
5. vag_tempered_run_dev is the composition of the building blocks, whatever the chunk size; thinning; the smallest ladder;
6. one rung is the plain device sampler;
7. upper limits and a noise group with a free sys_<label> pass through;
8. Fitter.fit(sampler="tempered") end to end;
9. the refusals of the raw C-ABI, the context usable afterwards, device memory back after vag_ctx_destroy;
10. the new symbols."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_gpu_parity as tg
import test_limits as tl
import test_sky_visfit as tv
import test_tempering_host as th
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu

P = fitting.ParamDef
defs, TRUTH, new_fitter = tc.defs, tc.TRUTH, tc.new_fitter
PRIORS = {"theta_v": ("gaussian", 0.4, 0.05)}  # one free parameter with a prior that is not flat


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def c4_data():
    """Flux-density rows on C4_EPOCHS at the three C4_BANDS: the device's own flux at TRUTH times exp(0.1 N(0, 1)), 10 % errors."""
    t, nu = configs.c4_mock_data()  # (ascending in t, as a series request wants them)
    flux = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], t, nu)[0]
    assert np.all(flux > 0) and np.all(np.isfinite(flux))
    obs = flux * np.exp(0.1 * np.random.default_rng(2024).standard_normal(t.size))
    return [(b, t[nu == b], obs[nu == b], 0.1 * obs[nu == b]) for b in configs.C4_BANDS]


@pytest.fixture(scope="module")
def c4(c4_data):
    f = new_fitter()
    for b, t, obs, err in c4_data:
        f.add_flux_density(b, t, obs, err)
    return f


def start(f, d, ntemps, nw, center, seed=11):
    _, lo, hi = f.build_spec(d)
    pos = sampling.initial_positions(lo, hi, ntemps * nw, np.random.default_rng(seed), center=center, spread=0.02)
    return pos.reshape(ntemps, nw, -1), lo, hi


def composed(torch, f, d, pos0, betas, nsteps, seed, priors=None):
    """The run as a Python loop of the building blocks around vag_loglike_split_dev:
    (chain, lnl, lnprior, accepted counts, swapped counts)."""
    T, nw, ndim = pos0.shape
    move = sampling.TemperedMove(betas, nw, ndim, seed=seed)
    spec, _, _ = f.build_spec(d, priors=priors, use_priors=True)
    pos = torch.from_numpy(pos0).cuda()
    lnl = torch.empty((T, nw), dtype=torch.float64, device=pos.device)
    lnprior = torch.empty_like(lnl)
    sampling.loglike_split_device(f, spec, pos.view(-1, ndim), lnl.view(-1), lnprior.view(-1))
    accepted = torch.zeros((T, nw), dtype=torch.int64, device=pos.device)
    swapped = torch.zeros((max(T - 1, 1), nw), dtype=torch.int64, device=pos.device)
    lnl_new = torch.empty((T, nw // 2), dtype=torch.float64, device=pos.device)
    lnprior_new = torch.empty_like(lnl_new)
    chain, l_chain, p_chain = [], [], []
    for step in range(nsteps):
        for half in (0, 1):
            prop = move.propose(step, half, pos)
            sampling.loglike_split_device(f, spec, prop.view(-1, ndim), lnl_new.view(-1), lnprior_new.view(-1))
            move.accept(step, half, prop, lnl_new, lnprior_new, pos, lnl, lnprior, accepted)
        move.swap(step, pos, lnl, lnprior, swapped)
        chain.append(pos.cpu().numpy())
        l_chain.append(lnl.cpu().numpy())
        p_chain.append(lnprior.cpu().numpy())
    return np.array(chain), np.array(l_chain), np.array(p_chain), accepted.cpu().numpy(), swapped.cpu().numpy()


def swap_counts(run, ntemps, nw, nsteps, step0=0):
    """The accepted exchanges per pair of a run's swap_fraction."""
    return np.rint(run[4] * sampling.swap_attempts(ntemps, step0, nsteps) * nw).astype(np.int64)


# ---------------------------------------------------------------- 1. proposal bits
# (3, 130, 3): a half of 65 and T 65 = 195 items straddle wavefronts and the 256-lane group; (64, 34, 16): the longest ladder
@pytest.mark.parametrize("ntemps,nw,ndim", [(1, 4, 1), (2, 4, 2), (3, 130, 3), (64, 34, 16)])
def test_proposals_are_the_host_statement_to_the_bit(torch, ntemps, nw, ndim):
    pos = np.random.default_rng(1).standard_normal((ntemps, nw, ndim)) * np.logspace(-3, 3, ndim)
    d_pos = torch.from_numpy(pos).cuda()
    betas = sampling.geometric_betas(ntemps, 1e-3)
    for seed in (0, 2 ** 40 + 7):
        for a in (2.0, 1.5):
            move = sampling.TemperedMove(betas, nw, ndim, seed=seed, a=a)
            for step in (0, 1, 2 ** 32 + 5):
                for half in (0, 1):
                    got = move.propose(step, half, d_pos).cpu().numpy()
                    want, z, partner = sampling.tempered_proposals(pos, step, half, seed, a)
                    assert got.shape == (ntemps, nw // 2, ndim)
                    assert np.array_equal(got, want), (seed, a, step, half, np.abs(got - want).max())
                    assert np.all((z >= 1 / a) & (z < a)) and np.all(partner // (nw // 2) == 1 - half)
    assert np.array_equal(d_pos.cpu().numpy(), pos)  # proposing moves nothing


# ---------------------------------------------------------------- 2. decisions, exchanges and chain bits
def test_decisions_swaps_and_chain_are_the_host_statement_to_the_bit(torch):
    T, nw, nsteps, seed = 4, 32, 300, 1
    betas = sampling.geometric_betas(T, 1e-3)
    pos0 = th.bimodal_start(T, nw, seed)
    margins = []
    chain, lnl_c, lnprior_c, acc, swap_fraction = sampling.run_tempered_philox(th.bimodal_log_like, th.box_log_prior, pos0, betas, nsteps,
                                                                              seed=seed, margins=margins)
    assert np.abs(th.all_margins(margins)).min() > 1e-9  # the condition under which every decision is compared
    move = sampling.TemperedMove(betas, nw, 2, seed=seed)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    pos = up(pos0)
    lnl, lnprior = up(th.bimodal_log_like(pos0.reshape(-1, 2)).reshape(T, nw)), up(th.box_log_prior(pos0.reshape(-1, 2)).reshape(T, nw))
    accepted = torch.zeros((T, nw), dtype=torch.int64, device=dev)
    swapped = torch.zeros((T - 1, nw), dtype=torch.int64, device=dev)
    was_hot = np.zeros((T, nw), dtype=bool)  # the state now at (t, w) has been at the hottest rung
    was_hot[T - 1] = True
    before = np.zeros((T - 1, nw), dtype=np.int64)
    parities, arrivals = set(), 0
    for step in range(nsteps):
        for half in (0, 1):
            prop = move.propose(step, half, pos)
            flat = prop.cpu().numpy().reshape(-1, 2)
            move.accept(step, half, prop, up(th.bimodal_log_like(flat).reshape(T, nw // 2)), up(th.box_log_prior(flat).reshape(T, nw // 2)),
                        pos, lnl, lnprior, accepted)
        move.swap(step, pos, lnl, lnprior, swapped)
        assert np.array_equal(pos.cpu().numpy(), chain[step]) and np.array_equal(lnl.cpu().numpy(), lnl_c[step]), step
        assert np.array_equal(lnprior.cpu().numpy(), lnprior_c[step]), step
        now = swapped.cpu().numpy()
        moved = now - before
        before = now
        assert set(np.unique(moved)) <= {0, 1} and not moved[(1 - step % 2)::2].any()  # only the pairs with t + step even
        if moved.any():
            parities.add(step % 2)
        cold_before = was_hot[0].copy()
        for t in range(step % 2, T - 1, 2):
            w = moved[t] == 1
            was_hot[t, w], was_hot[t + 1, w] = was_hot[t + 1, w].copy(), was_hot[t, w].copy()
        arrivals += int((was_hot[0] & ~cold_before).sum())
        was_hot[T - 1] = True
    assert np.array_equal(accepted.cpu().numpy(), np.rint(acc * nsteps).astype(np.int64))
    assert np.array_equal(before.sum(axis=1), swap_counts((None,) * 4 + (swap_fraction,), T, nw, nsteps))
    assert parities == {0, 1}
    assert arrivals > 0  # a state that was at the hottest rung reached the cold one
    assert 0.2 < acc[0].mean() < 0.8 and np.all(swap_fraction > 0.1)


# ---------------------------------------------------------------- 3. not finite: rejected
@pytest.mark.parametrize("beta_hot", [0.5, 0.0])
def test_a_proposal_that_is_not_finite_is_rejected_at_every_temperature(torch, beta_hot):
    """NaN, +inf and -inf in ln L or in ln prior are rejected whatever the draw and whatever beta (0 too, where ln L does not enter
    the ratio); a huge finite value is decided like any other -- taken where beta > 0 or where it is the prior's."""
    T, nw, ndim = 2, 8, 2
    betas = [1.0, beta_hot]
    move = sampling.TemperedMove(betas, nw, ndim, seed=9)
    pos0 = np.random.default_rng(3).standard_normal((T, nw, ndim))
    dev = torch.device("cuda", 0)
    bad = np.tile(np.array([np.nan, np.inf, -np.inf, 1e300]), (T, 1))
    zero = np.zeros((T, 4))
    for half in (0, 1):
        for l_new, p_new in ((bad, zero), (zero, bad)):
            pos = torch.from_numpy(pos0).to(dev)
            lnl = torch.zeros((T, nw), dtype=torch.float64, device=dev)
            lnprior = torch.zeros((T, nw), dtype=torch.float64, device=dev)
            accepted = torch.zeros((T, nw), dtype=torch.int64, device=dev)
            prop = move.propose(4, half, pos)
            move.accept(4, half, prop, torch.from_numpy(l_new).to(dev), torch.from_numpy(p_new).to(dev), pos, lnl, lnprior, accepted)
            z = sampling.tempered_proposals(pos0, 4, half, 9)[1]
            take, margin = sampling.tempered_accepts(4, half, 9, z, betas, l_new, p_new, zero, zero, ndim)
            assert not take[:, :3].any() and np.abs(margin[:, 3]).min() > 1e-9
            assert take[0, 3] and (take[1, 3] or (beta_hot == 0.0 and l_new is bad))
            s = slice(half * 4, half * 4 + 4)
            want_pos, want_l, want_p = pos0.copy(), np.zeros((T, nw)), np.zeros((T, nw))
            want_acc = np.zeros((T, nw), dtype=np.int64)
            want_pos[:, s][take] = prop.cpu().numpy()[take]
            want_l[:, s][take], want_p[:, s][take] = l_new[take], p_new[take]
            want_acc[:, s][take] = 1
            assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(accepted.cpu().numpy(), want_acc)
            assert np.array_equal(lnl.cpu().numpy(), want_l) and np.array_equal(lnprior.cpu().numpy(), want_p)


# ---------------------------------------------------------------- 4. ln L and ln prior apart
def test_split_is_the_likelihood_call_taken_apart(c4):
    d = defs()
    _, lo, hi = c4.build_spec(d)
    walkers = {}
    for nb, seed in ((130, 21), (5, 22)):  # (130: from 64 walkers on a repeated call evaluates in cost order; 5: never)
        x = sampling.initial_positions(lo, hi, nb, np.random.default_rng(seed), center=TRUTH, spread=0.05)
        x[1, 0], x[2, 1], x[4, 2] = hi[0] + 0.01, lo[1] - 0.1, hi[2] + 1.0  # three walkers outside the box
        walkers[nb] = x
    got = {}
    for nb in (130, 130, 5, 5, 130):  # the second and the last call of 130 evaluate in the order the one before left
        lnl, lnprior = c4.log_like_and_prior_batch(walkers[nb], d, priors=PRIORS)
        assert lnl.shape == lnprior.shape == (nb,)
        if nb in got:  # a second call, whatever the size of the call between, gives the same bits
            assert np.array_equal(lnl, got[nb][0]) and np.array_equal(lnprior, got[nb][1])
        got[nb] = (lnl, lnprior)
    for nb, x in walkers.items():
        lnl, lnprior = got[nb]
        lp = c4.log_prob_batch(x, d, priors=PRIORS)
        inside = np.all((x >= lo) & (x <= hi), axis=1)
        assert inside.sum() == nb - 3 and np.all(np.isfinite(lp[inside])) and np.all(lp[~inside] == -np.inf)
        assert np.array_equal((lnl + lnprior)[inside], lp[inside])
        assert np.all((lnl + lnprior)[~inside] == -np.inf) and np.all(lnprior[~inside] == -np.inf)
        assert np.array_equal(lnl[inside], c4.loglike_batch(x[inside], d))
        # the prior is the Gaussian of theta_v plus the flat ones: not a constant
        flat = c4.log_like_and_prior_batch(x, d)[1]
        want = flat[inside] - 0.5 * ((x[inside, 1] - 0.4) / 0.05) ** 2 - np.log(0.05 * np.sqrt(2 * np.pi))
        assert np.ptp(lnprior[inside]) > 0.1 and np.allclose(lnprior[inside] - want, (lnprior[inside] - want)[0], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 5. vag_tempered_run_dev is the composition
BETAS3 = [1.0, 0.3, 0.0]


@pytest.fixture(scope="module")
def run130(torch, c4):
    d = defs()
    pos0, lo, hi = start(c4, d, 3, 130, TRUTH)
    return dict(d=d, pos0=pos0, lo=lo, hi=hi, run=sampling.run_tempered_device(c4, d, pos0, BETAS3, 6, seed=5, chunk=6, priors=PRIORS))


def test_run_is_the_composition_of_the_building_blocks(torch, c4, run130):
    chain, lnl, lnprior, acc, swap_fraction = run130["run"]
    assert chain.shape == (6, 3, 130, 3) and lnl.shape == lnprior.shape == (6, 3, 130) and acc.shape == (3, 130)
    assert swap_fraction.shape == (2,)
    want = composed(torch, c4, run130["d"], run130["pos0"], BETAS3, 6, seed=5, priors=PRIORS)
    assert np.array_equal(chain, want[0]) and np.array_equal(lnl, want[1]) and np.array_equal(lnprior, want[2])
    assert np.array_equal(np.rint(acc * 6).astype(np.int64), want[3]) and 0 < want[3].sum() < 6 * 3 * 130
    assert np.array_equal(swap_counts(run130["run"], 3, 130, 6), want[4][:2].sum(axis=1)) and want[4].sum() > 0
    assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnprior))
    assert np.all(chain >= run130["lo"]) and np.all(chain <= run130["hi"])  # the prior rung too
    # positions and what is stored with them belong together
    last = chain[-1].reshape(-1, 3)
    assert np.array_equal((lnl[-1] + lnprior[-1]).ravel(), c4.log_prob_batch(last, run130["d"], priors=PRIORS))


@pytest.mark.parametrize("chunk", [4, 1])
def test_chunks_do_not_change_a_bit(c4, run130, chunk):
    seen = []
    got = sampling.run_tempered_device(c4, run130["d"], run130["pos0"], BETAS3, 6, seed=5, chunk=chunk, priors=PRIORS,
                                       progress=lambda step, pos, lnl, lnprior: seen.append((step, pos.copy(), lnl.copy(), lnprior.copy())))
    assert all(np.array_equal(g, w) for g, w in zip(got, run130["run"]))
    assert [s[0] for s in seen] == ([3, 5] if chunk == 4 else list(range(6)))
    assert all(np.array_equal(pos, got[0][s]) and np.array_equal(l, got[1][s]) and np.array_equal(p, got[2][s]) for s, pos, l, p in seen)


def test_thin_keeps_every_second_step(c4, run130):
    got = sampling.run_tempered_device(c4, run130["d"], run130["pos0"], BETAS3, 6, seed=5, thin=2, chunk=4, priors=PRIORS)
    assert got[0].shape == (3, 3, 130, 3)
    assert all(np.array_equal(g, w[1::2]) for g, w in zip(got[:3], run130["run"][:3]))
    assert np.array_equal(got[3], run130["run"][3]) and np.array_equal(got[4], run130["run"][4])


def test_smallest_ladder_is_the_composition(torch, c4):
    """Two temperatures of 4 walkers, one free parameter: 4 proposals per call, below the 64 from which the engine reorders."""
    d = [P("theta_c", 0.02, 0.3)] + tv._c4_fixed(skip=("theta_c",))
    pos0, lo, hi = start(c4, d, 2, 4, TRUTH[:1])
    got = sampling.run_tempered_device(c4, d, pos0, [1.0, 0.2], 6, seed=5, chunk=4)
    want = composed(torch, c4, d, pos0, [1.0, 0.2], 6, seed=5)
    assert got[0].shape == (6, 2, 4, 1)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
    assert np.array_equal(np.rint(got[3] * 6).astype(np.int64), want[3])
    assert np.array_equal(swap_counts(got, 2, 4, 6), want[4][:1].sum(axis=1))
    assert np.array_equal((got[1][-1] + got[2][-1]).ravel(), c4.log_prob_batch(got[0][-1].reshape(-1, 1), d))
    assert np.all(got[0] >= lo) and np.all(got[0] <= hi)


# ---------------------------------------------------------------- 6. one rung is the plain device sampler
def test_one_rung_is_the_plain_device_sampler(c4):
    """betas = [1]: the same counters, and a ratio fma(1, lnL' - lnL, lnpi' - lnpi) that differs from (lnL' + lnpi') - (lnL + lnpi)
    by roundings of order 1e-14, against margins of order 1e-6 and larger: the same positions."""
    d = defs()
    pos0, _, _ = start(c4, d, 1, 130, TRUTH)
    chain, lnl, lnprior, acc, swap_fraction = sampling.run_tempered_device(c4, d, pos0, [1.0], 6, seed=5)
    plain_chain, plain_logp, plain_acc = sampling.run_stretch_move_device(c4, d, pos0[0], 6, seed=5)
    assert np.array_equal(chain[:, 0], plain_chain) and np.array_equal(acc[0], plain_acc) and swap_fraction.shape == (0,)
    assert np.array_equal(lnl[:, 0] + lnprior[:, 0], plain_logp)  # (the call's own sum, to the bit)


# ---------------------------------------------------------------- 7. data kinds pass through
def test_limits_and_noise_groups_pass_through(c4_data):
    f = new_fitter()
    for k, (b, t, obs, err) in enumerate(c4_data):
        lim = np.zeros(t.size, dtype=bool)
        lim[7] = k == 1  # one upper-limit row, 3 sigma above the datum
        value = np.where(lim, 1.3 * obs, obs)
        f.add_flux_density(b, t, value, err, upper_limit=lim if k == 1 else None, noise="radio" if k == 0 else None)
    assert f.has_limits and f.has_noise_groups
    d = defs([P("sys_radio", 0.0, 0.5)])
    pos0, lo, hi = start(f, d, 2, 64, np.append(TRUTH, 0.1))
    chain, lnl, lnprior, acc, swap_fraction = sampling.run_tempered_device(f, d, pos0, [1.0, 0.1], 3, seed=1)
    assert chain.shape == (3, 2, 64, 4) and np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnprior))
    assert np.all(chain >= lo) and np.all(chain <= hi) and acc.sum() > 0
    again = f.log_like_and_prior_batch(chain[-1].reshape(-1, 4), d)
    assert np.array_equal(lnl[-1].ravel(), again[0]) and np.array_equal(lnprior[-1].ravel(), again[1])


# ---------------------------------------------------------------- 8. end to end
def test_end_to_end_fit_with_the_tempered_sampler(oracle):
    """The assertions of test_end_to_end_fit_with_the_device_sampler on its problem, on the cold chain of a ladder of four."""
    f, d = tg._c4_fitter(oracle)
    _, lo, hi = f.build_spec(d)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    ll_truth = f.loglike_batch(truth[None, :], d)[0]
    res = f.fit(d, nwalkers=32, nsteps=40, nburn=20, seed=1, sampler="tempered", ntemps=4, center=truth + 0.05 * (hi - lo), spread=0.02)
    assert res["samples"].shape == (20 * 32, len(d)) and np.all(np.isfinite(res["log_prob"]))
    assert np.all(res["samples"] >= lo) and np.all(res["samples"] <= hi)
    assert res["log_prob"].max() > ll_truth - 40
    assert res["chain"].shape == (40, 32, len(d)) and res["chain"][-1].std(axis=0).min() > 0
    assert res["acceptance"].shape == (32,) and 0.05 < res["acceptance"].mean() < 0.95
    assert np.isfinite(res["log_evidence"]) and np.isfinite(res["log_evidence_error"])
    assert res["betas"].shape == (4,) and res["betas"][0] == 1.0 and res["betas"][-1] == 0.0 and res["swap_fraction"].shape == (3,)
    print("mean ln L per rung", res["log_like"], "ln Z", res["log_evidence"], "+-", res["log_evidence_error"])
    assert res["log_like"].shape == (4,) and res["log_like"][0] > res["log_like"][-1]


# ---------------------------------------------------------------- 9. the raw C-ABI: refusals, the context afterwards, memory
def test_refusals_leave_the_context_usable_and_memory_returns(torch, c4):
    lib = _lib.load()
    d = defs()
    spec, _, _ = c4.build_spec(d, use_priors=True)
    request = fitting.loglike_request(spec)
    T, nw, ndim, nsteps = 3, 8, 3, 2
    pos0, _, _ = start(c4, d, T, nw, TRUTH)
    lnl0, lnprior0 = c4.log_like_and_prior_batch(pos0.reshape(-1, ndim), d)
    assert np.all(np.isfinite(lnl0)) and np.all(np.isfinite(lnprior0))
    dev = torch.device("cuda", 0)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    dp = C.POINTER(C.c_double)
    ladders = []  # (kept alive: the specs point into them)

    def sp_with(betas=(1.0, 0.3, 0.0), **kw):
        arr = np.array(betas, dtype=np.float64) if betas is not None else None
        ladders.append(arr)
        s = _lib.TemperedSpec(5, 2.0, len(betas) if betas is not None else 3, nw, ndim, 1, arr.ctypes.data_as(dp) if arr is not None else None)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    good = sp_with()
    ref = C.byref
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731

    def buffers():
        b = dict(pos=torch.from_numpy(pos0).to(dev), lnl=torch.from_numpy(lnl0.reshape(T, nw)).to(dev),
                 lnprior=torch.from_numpy(lnprior0.reshape(T, nw)).to(dev), acc=zeros(T, nw, dtype=torch.int64),
                 swp=zeros(T - 1, nw, dtype=torch.int64), chain=zeros(nsteps, T, nw, ndim), lchain=zeros(nsteps, T, nw),
                 pchain=zeros(nsteps, T, nw), prop=zeros(T, nw // 2, ndim), l_new=zeros(T, nw // 2), p_new=zeros(T, nw // 2))
        torch.cuda.synchronize()  # (the context runs on a stream of its own)
        return b

    def run(b, ctx=ctx, request=request, sp=good, n=nsteps, **null):
        p = {k: (None if k in null else v.data_ptr()) for k, v in b.items()}
        rc = lib.vag_tempered_run_dev(ctx, ref(request) if request is not None else None, ref(sp) if sp is not None else None, 0, n,
                                      p["pos"], p["lnl"], p["lnprior"], p["acc"], p["swp"], p["chain"], p["lchain"], p["pchain"])
        if ctx is not None:
            _lib.check(lib.vag_ctx_synchronize(ctx))
        return rc

    def state(b):
        return [b[k].cpu().numpy() for k in ("pos", "lnl", "lnprior", "acc", "swp", "chain", "lchain", "pchain")]

    b = buffers()
    assert run(b) == _lib.VAG_OK
    first = state(b)
    assert np.array_equal(first[0], first[5][-1]) and np.array_equal(first[1], first[6][-1]) and np.array_equal(first[2], first[7][-1])
    assert np.all(np.isfinite(first[6])) and np.all(np.isfinite(first[7]))
    # ... and it is the run of the Python driver
    want = sampling.run_tempered_device(c4, d, pos0, [1.0, 0.3, 0.0], nsteps, seed=5)
    assert np.array_equal(first[5], want[0]) and np.array_equal(first[6], want[1]) and np.array_equal(first[7], want[2])

    def refused(rc, what):
        assert rc == _lib.VAG_E_INVALID, what
        msg = _lib.last_error()
        assert msg, what
        return msg

    no_spec = _lib.LoglikeRequest()  # every block null
    long_ladder = tuple(np.linspace(1.0, 0.0, 65))
    bad_specs = [("odd", sp_with(n_walkers=7)), ("few", sp_with(n_walkers=4)), ("ndim 0", sp_with(ndim=0)),
                 ("ndim 17", sp_with(ndim=17, n_walkers=40)), ("a nan", sp_with(a=float("nan"))), ("a inf", sp_with(a=float("inf"))),
                 ("a 1", sp_with(a=1.0)), ("a 0.5", sp_with(a=0.5)), ("thin 0", sp_with(thin=0)),
                 ("no temperature", sp_with(n_temps=0)), ("n_temps < 0", sp_with(n_temps=-1)), ("65 temperatures", sp_with(long_ladder)),
                 ("null betas", sp_with(None)), ("betas[0] != 1", sp_with((0.9, 0.3, 0.0))), ("betas[0] > 1", sp_with((1.5, 1.0, 0.0))),
                 ("equal rungs", sp_with((1.0, 0.3, 0.3))), ("ascending rung", sp_with((1.0, 0.3, 0.5))),
                 ("negative rung", sp_with((1.0, 0.3, -0.1))), ("nan rung", sp_with((1.0, float("nan"), 0.0))),
                 ("-inf rung", sp_with((1.0, 0.3, float("-inf"))))]
    fresh = buffers()
    untouched = state(fresh)
    for what, rc in [("null context", run(fresh, ctx=None)), ("null request", run(fresh, request=None)),
                     ("null fit spec", run(fresh, request=no_spec)), ("null tempered spec", run(fresh, sp=None)),
                     ("null pos", run(fresh, pos=1)), ("null lnl", run(fresh, lnl=1)), ("null lnprior", run(fresh, lnprior=1)),
                     ("null accepted", run(fresh, acc=1)), ("null swapped", run(fresh, swp=1)),
                     ("chain alone missing", run(fresh, chain=1)), ("lnl chain alone missing", run(fresh, lchain=1)),
                     ("lnprior chain alone missing", run(fresh, pchain=1)), ("chain alone given", run(fresh, lchain=1, pchain=1)),
                     ("ndim of another fit", run(fresh, sp=sp_with(ndim=2))), ("n_steps < 0", run(fresh, n=-1))] + \
                    [(what, run(fresh, sp=s)) for what, s in bad_specs]:
        refused(rc, what)
    p = {k: v.data_ptr() for k, v in fresh.items()}
    accept_args = [p["prop"], p["l_new"], p["p_new"], p["pos"], p["lnl"], p["lnprior"], p["acc"]]
    swap_args = [p["pos"], p["lnl"], p["lnprior"], p["swp"]]
    for what, s in bad_specs + [("null", None)]:
        sp = ref(s) if s is not None else None
        refused(lib.vag_tempered_propose_dev(ctx, sp, 0, 0, p["pos"], p["prop"]), "propose: " + what)
        refused(lib.vag_tempered_accept_dev(ctx, sp, 0, 0, *accept_args), "accept: " + what)
        refused(lib.vag_tempered_swap_dev(ctx, sp, 0, *swap_args), "swap: " + what)
    for half in (-1, 2):
        assert "half" in refused(lib.vag_tempered_propose_dev(ctx, ref(good), 0, half, p["pos"], p["prop"]), "propose: half")
        assert "half" in refused(lib.vag_tempered_accept_dev(ctx, ref(good), 0, half, *accept_args), "accept: half")
    refused(lib.vag_tempered_propose_dev(None, ref(good), 0, 0, p["pos"], p["prop"]), "propose: null context")
    refused(lib.vag_tempered_propose_dev(ctx, ref(good), 0, 0, None, p["prop"]), "propose: null pos")
    refused(lib.vag_tempered_propose_dev(ctx, ref(good), 0, 0, p["pos"], None), "propose: null prop")
    refused(lib.vag_tempered_accept_dev(None, ref(good), 0, 0, *accept_args), "accept: null context")
    refused(lib.vag_tempered_swap_dev(None, ref(good), 0, *swap_args), "swap: null context")
    for k in range(7):
        args = list(accept_args)
        args[k] = None
        refused(lib.vag_tempered_accept_dev(ctx, ref(good), 0, 0, *args), f"accept: null buffer {k}")
    for k in range(4):
        args = list(swap_args)
        args[k] = None
        refused(lib.vag_tempered_swap_dev(ctx, ref(good), 0, *args), f"swap: null buffer {k}")
    theta = torch.from_numpy(pos0.reshape(-1, ndim)).to(dev)
    split_args = [theta.data_ptr(), T * nw, ndim, p["lnl"], p["lnprior"]]
    refused(lib.vag_loglike_split_dev(None, ref(request), *split_args), "split: null context")
    refused(lib.vag_loglike_split_dev(ctx, None, *split_args), "split: null request")
    refused(lib.vag_loglike_split_dev(ctx, ref(no_spec), *split_args), "split: null fit spec")
    for k in (0, 3, 4):
        args = list(split_args)
        args[k] = None
        refused(lib.vag_loglike_split_dev(ctx, ref(request), *args), f"split: null pointer {k}")
    refused(lib.vag_loglike_split_dev(ctx, ref(request), theta.data_ptr(), 0, ndim, p["lnl"], p["lnprior"]), "split: empty batch")
    assert run(fresh, n=0) == _lib.VAG_OK  # no step: nothing happens
    _lib.check(lib.vag_ctx_synchronize(ctx))
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), untouched))
    # the context serves the valid call as before, and a run without a stored chain leaves the same state
    assert run(fresh) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), first))
    bare = buffers()
    assert run(bare, chain=1, lchain=1, pchain=1) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(bare)[:5], first[:5])) and not state(bare)[5].any()
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


# ---------------------------------------------------------------- 10. the new symbols
def test_new_symbols_are_exported_and_the_abi_stays_13():
    lib = _lib.load()
    for name in _lib.TEMPERED_ENTRIES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert _lib.tempered_entry(lib, name) is getattr(lib, name)
    assert lib.vag_abi_version() == 13
    assert _lib.TEMPER_MAX == sampling.TEMPER_MAX == 64
