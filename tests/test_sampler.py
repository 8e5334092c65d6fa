"""The ensemble sampler on the device (vag_stretch_propose_dev / _accept_dev / _run_dev; sampling.StretchMove,
run_stretch_move_device, fit(sampler="device")) against its numpy statement (sampling.stretch_proposals, stretch_accepts,
run_stretch_move_philox).  Everything is compared with np.array_equal: the proposals are fused operations and one IEEE division, and
the decisions of the runs compared here are all further than 1e-9 from their thresholds (asserted), far above the rounding of a
logarithm.

1. proposal bits over sizes, halves, steps beyond 2^32, seeds beyond 2^32 and two scales;
2. decisions and chain bits on the Gaussian of tests/test_sampler_host.py, ln p formed on the host;
3. vag_stretch_run_dev is the composition propose -> likelihood -> accept, whatever the chunk size; thinning; positions and stored
   ln p belong together; the smallest ensemble;
4. upper limits and a noise group with a free sys_<label> pass through; a proposal outside the box is never accepted;
5. Fitter.fit(sampler="device") end to end;
6. the refusals of the raw C-ABI, the context usable afterwards, device memory back after vag_ctx_destroy."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_gpu_parity as tg
import test_index as ti
import test_limits as tl
import test_sampler_host as sh
import test_sky_visfit as tv
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu

P = fitting.ParamDef
defs, TRUTH, new_fitter = tc.defs, tc.TRUTH, ti.new_fitter


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


def start(f, d, nw, center, seed=11):
    _, lo, hi = f.build_spec(d)
    return sampling.initial_positions(lo, hi, nw, np.random.default_rng(seed), center=center, spread=0.02), lo, hi


def composed(torch, f, d, pos0, nsteps, seed, a=2.0):
    """The run as a Python loop of the building blocks around Fitter.device_evaluator: (chain, logp, accepted counts)."""
    nw, ndim = pos0.shape
    move = sampling.StretchMove(nw, ndim, seed=seed, a=a)
    eval_dev = f.device_evaluator(d, use_priors=True)
    pos = torch.from_numpy(pos0).cuda()
    lp = eval_dev(pos, want_costs=False)[0]
    accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
    chain, logp = [], []
    for step in range(nsteps):
        for half in (0, 1):
            prop = move.propose(step, half, pos)
            move.accept(step, half, prop, eval_dev(prop, want_costs=False)[0], pos, lp, accepted)
        chain.append(pos.cpu().numpy())
        logp.append(lp.cpu().numpy())
    return np.array(chain), np.array(logp), accepted.cpu().numpy()


# ---------------------------------------------------------------- 1. proposal bits
@pytest.mark.parametrize("nw,ndim", [(4, 1), (4, 2), (130, 3), (130, 16)])  # (130: the half of 65 straddles a wavefront)
def test_proposals_are_the_host_statement_to_the_bit(torch, nw, ndim):
    pos = np.random.default_rng(1).standard_normal((nw, ndim)) * np.logspace(-3, 3, ndim)
    d_pos = torch.from_numpy(pos).cuda()
    for seed in (0, 2 ** 40 + 7):
        for a in (2.0, 1.5):
            move = sampling.StretchMove(nw, ndim, seed=seed, a=a)
            for step in (0, 1, 2 ** 32 + 5):
                for half in (0, 1):
                    got = move.propose(step, half, d_pos).cpu().numpy()
                    want, z, partner = sampling.stretch_proposals(pos, step, half, seed, a)
                    assert got.shape == (nw // 2, ndim)
                    assert np.array_equal(got, want), (seed, a, step, half, np.abs(got - want).max())
                    assert np.all((z >= 1 / a) & (z < a)) and np.all(partner // (nw // 2) == 1 - half)
    assert np.array_equal(d_pos.cpu().numpy(), pos)  # proposing moves nothing


# ---------------------------------------------------------------- 2. decisions and chain bits
def test_decisions_and_chain_are_the_host_statement_to_the_bit(torch):
    nsteps, seed, pos0 = 300, sh.GAUSS_SEED, sh.gaussian_start()
    margins = []
    chain, logp, acc = sampling.run_stretch_move_philox(sh.gaussian_log_prob, pos0, nsteps, seed=seed, margins=margins)
    assert np.abs(np.concatenate(margins)).min() > 1e-9  # the condition of the host test: every decision is compared
    nw, ndim = pos0.shape
    move = sampling.StretchMove(nw, ndim, seed=seed)
    pos = torch.from_numpy(pos0).cuda()
    lp = torch.from_numpy(sh.gaussian_log_prob(pos0)).cuda()
    accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
    for step in range(nsteps):
        for half in (0, 1):
            prop = move.propose(step, half, pos)
            lp_new = torch.from_numpy(sh.gaussian_log_prob(prop.cpu().numpy())).cuda()
            move.accept(step, half, prop, lp_new, pos, lp, accepted)
        assert np.array_equal(pos.cpu().numpy(), chain[step]) and np.array_equal(lp.cpu().numpy(), logp[step]), step
    assert np.array_equal(accepted.cpu().numpy(), np.rint(acc * nsteps).astype(np.int64))
    assert 0.4 < acc.mean() < 0.9


def test_a_proposal_that_is_not_finite_is_rejected(torch):
    """NaN, +inf and -inf are rejected whatever the draw; a huge finite ln p is taken; log(u) is compared, not u."""
    nw, ndim = 8, 2
    move = sampling.StretchMove(nw, ndim, seed=9)
    pos0 = np.random.default_rng(3).standard_normal((nw, ndim))
    for half in (0, 1):
        pos = torch.from_numpy(pos0).cuda()
        lp = torch.zeros(nw, dtype=torch.float64, device=pos.device)
        accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
        prop = move.propose(4, half, pos)
        lp_new = torch.tensor([np.nan, np.inf, -np.inf, 1e300], dtype=torch.float64, device=pos.device)
        move.accept(4, half, prop, lp_new, pos, lp, accepted)
        s = slice(half * 4, half * 4 + 4)
        want_pos, want_lp = pos0.copy(), np.zeros(nw)
        want_pos[s][3], want_lp[s][3] = prop.cpu().numpy()[3], 1e300
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(lp.cpu().numpy(), want_lp)
        assert accepted.cpu().numpy()[s].tolist() == [0, 0, 0, 1] and accepted.cpu().numpy().sum() == 1


# ---------------------------------------------------------------- 3. vag_stretch_run_dev is the composition
@pytest.fixture(scope="module")
def run130(torch, c4):
    d = defs()
    pos0, lo, hi = start(c4, d, 130, TRUTH)
    return dict(d=d, pos0=pos0, lo=lo, hi=hi, run=sampling.run_stretch_move_device(c4, d, pos0, 6, seed=5, chunk=6))


def test_run_is_the_composition_of_the_building_blocks(torch, c4, run130):
    chain, logp, acc = run130["run"]
    assert chain.shape == (6, 130, 3) and logp.shape == (6, 130) and acc.shape == (130,)
    want_chain, want_logp, want_count = composed(torch, c4, run130["d"], run130["pos0"], 6, seed=5)
    assert np.array_equal(chain, want_chain) and np.array_equal(logp, want_logp)
    assert np.array_equal(np.rint(acc * 6).astype(np.int64), want_count) and 0 < want_count.sum() < 6 * 130
    assert np.all(np.isfinite(logp)) and np.all(chain >= run130["lo"]) and np.all(chain <= run130["hi"])
    # positions and stored ln p belong together
    assert np.array_equal(logp[-1], c4.log_prob_batch(chain[-1], run130["d"]))


@pytest.mark.parametrize("chunk", [4, 1])
def test_chunks_do_not_change_a_bit(c4, run130, chunk):
    seen = []
    got = sampling.run_stretch_move_device(c4, run130["d"], run130["pos0"], 6, seed=5, chunk=chunk,
                                           progress=lambda step, pos, lp: seen.append((step, pos.copy(), lp.copy())))
    assert all(np.array_equal(g, w) for g, w in zip(got, run130["run"]))
    assert [s for s, _, _ in seen] == ([3, 5] if chunk == 4 else list(range(6)))
    assert all(np.array_equal(pos, got[0][s]) and np.array_equal(lp, got[1][s]) for s, pos, lp in seen)


def test_thin_keeps_every_second_step(c4, run130):
    chain, logp, acc = sampling.run_stretch_move_device(c4, run130["d"], run130["pos0"], 6, seed=5, thin=2, chunk=4)
    assert chain.shape == (3, 130, 3)
    assert np.array_equal(chain, run130["run"][0][1::2]) and np.array_equal(logp, run130["run"][1][1::2])
    assert np.array_equal(acc, run130["run"][2])


def test_smallest_ensemble_is_the_composition(torch, c4):
    """4 walkers, one free parameter: halves of 2, below the 64 walkers from which the engine reorders its evaluation."""
    d = [P("theta_c", 0.02, 0.3)] + tv._c4_fixed(skip=("theta_c",))
    pos0, lo, hi = start(c4, d, 4, TRUTH[:1])
    chain, logp, acc = sampling.run_stretch_move_device(c4, d, pos0, 6, seed=5, chunk=4)
    want_chain, want_logp, want_count = composed(torch, c4, d, pos0, 6, seed=5)
    assert chain.shape == (6, 4, 1)
    assert np.array_equal(chain, want_chain) and np.array_equal(logp, want_logp)
    assert np.array_equal(np.rint(acc * 6).astype(np.int64), want_count)
    assert np.array_equal(logp[-1], c4.log_prob_batch(chain[-1], d)) and np.all(chain >= lo) and np.all(chain <= hi)


# ---------------------------------------------------------------- 4. data kinds pass through
def test_limits_and_noise_groups_pass_through(c4_data):
    f = new_fitter()
    for k, (b, t, obs, err) in enumerate(c4_data):
        lim = np.zeros(t.size, dtype=bool)
        lim[7] = k == 1  # one upper-limit row, 3 sigma above the datum
        value = np.where(lim, 1.3 * obs, obs)
        f.add_flux_density(b, t, value, err, upper_limit=lim if k == 1 else None, noise="radio" if k == 0 else None)
    assert f.has_limits and f.has_noise_groups
    d = defs([P("sys_radio", 0.0, 0.5)])
    center = np.append(TRUTH, 0.1)
    pos0, lo, hi = start(f, d, 64, center)
    pos0[0, 0] = lo[0] + 1e-9 * (hi[0] - lo[0])  # on the edge: what this walker proposes with z > 1 lies outside the box
    seed, nsteps, nh = 1, 3, 32
    chain, logp, acc = sampling.run_stretch_move_device(f, d, pos0, nsteps, seed=seed)
    assert np.all(np.isfinite(logp)) and np.all(chain >= lo) and np.all(chain <= hi)
    assert np.array_equal(logp[-1], f.log_prob_batch(chain[-1], d))
    # the proposals again on the host, from the chain: every walker either stays or takes its proposal, and one outside the box stays
    outside = []
    prev = pos0
    for step in range(nsteps):
        mid = np.concatenate([chain[step][:nh], prev[nh:]])  # after the first half-step
        for half, before in ((0, prev), (1, mid)):
            s = slice(half * nh, half * nh + nh)
            prop = sampling.stretch_proposals(before, step, half, seed)[0]
            stays, moves = np.all(chain[step][s] == before[s], axis=1), np.all(chain[step][s] == prop, axis=1)
            assert np.all(stays | moves), (step, half)
            out = np.any((prop < lo) | (prop > hi), axis=1)
            assert np.all(stays[out]), (step, half)
            outside.extend(prop[out])
        prev = chain[step]
    assert len(outside) > 0
    assert np.all(f.log_prob_batch(np.array(outside), d) == -np.inf)
    assert 0 < acc.sum()


# ---------------------------------------------------------------- 5. end to end
def test_end_to_end_fit_with_the_device_sampler(oracle):
    """The assertions of test_end_to_end_mcmc_on_the_device_likelihood on its problem, the sampler on the device."""
    f, d = tg._c4_fitter(oracle)
    _, lo, hi = f.build_spec(d)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    ll_truth = f.loglike_batch(truth[None, :], d)[0]
    res = f.fit(d, nwalkers=32, nsteps=40, nburn=20, seed=1, sampler="device", center=truth + 0.05 * (hi - lo), spread=0.02)
    assert res["samples"].shape == (20 * 32, len(d)) and np.all(np.isfinite(res["log_prob"]))
    assert np.all(res["samples"] >= lo) and np.all(res["samples"] <= hi)
    assert res["log_prob"].max() > ll_truth - 40
    assert res["chain"][-1].std(axis=0).min() > 0 and 0.05 < res["acceptance"].mean() < 0.95


# ---------------------------------------------------------------- 6. the raw C-ABI: refusals, the context afterwards, memory
def test_refusals_leave_the_context_usable_and_memory_returns(torch, c4):
    lib = _lib.load()
    d = defs()
    spec, _, _ = c4.build_spec(d, use_priors=True)
    request = fitting.loglike_request(spec)
    nw, ndim, nsteps = 8, 3, 2
    pos0, _, _ = start(c4, d, nw, TRUTH)
    lp0 = c4.log_prob_batch(pos0, d)
    assert np.all(np.isfinite(lp0))
    dev = torch.device("cuda", 0)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    good = _lib.StretchSpec(5, 2.0, nw, ndim, 1)
    ref = C.byref

    def buffers():
        b = dict(pos=torch.from_numpy(pos0).to(dev), lp=torch.from_numpy(lp0).to(dev),
                 acc=torch.zeros(nw, dtype=torch.int64, device=dev), chain=torch.zeros((nsteps, nw, ndim), dtype=torch.float64, device=dev),
                 logp=torch.zeros((nsteps, nw), dtype=torch.float64, device=dev), prop=torch.zeros((nw // 2, ndim), dtype=torch.float64, device=dev),
                 lp_new=torch.zeros(nw // 2, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()  # (the context runs on a stream of its own)
        return b

    def run(b, ctx=ctx, request=request, sp=good, n=nsteps, **null):
        p = {k: (None if k in null else v.data_ptr()) for k, v in b.items()}
        rc = lib.vag_stretch_run_dev(ctx, ref(request) if request is not None else None, ref(sp) if sp is not None else None, 0, n,
                                     p["pos"], p["lp"], p["acc"], p["chain"], p["logp"])
        if ctx is not None:
            _lib.check(lib.vag_ctx_synchronize(ctx))
        return rc

    def state(b):
        return [b[k].cpu().numpy() for k in ("pos", "lp", "acc", "chain", "logp")]

    b = buffers()
    assert run(b) == _lib.VAG_OK
    first = state(b)
    assert np.array_equal(first[0], first[3][-1]) and np.array_equal(first[1], first[4][-1]) and np.all(np.isfinite(first[4]))

    def refused(rc, what):
        assert rc == _lib.VAG_E_INVALID, what
        msg = _lib.last_error()
        assert msg, what
        return msg

    def sp_with(**kw):
        s = _lib.StretchSpec(5, 2.0, nw, ndim, 1)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    no_spec = _lib.LoglikeRequest()  # every block null
    bad_specs = [("odd", sp_with(n_walkers=7)), ("few", sp_with(n_walkers=4)), ("ndim 0", sp_with(ndim=0)),
                 ("ndim 17", sp_with(ndim=17, n_walkers=40)), ("a nan", sp_with(a=float("nan"))), ("a inf", sp_with(a=float("inf"))),
                 ("a 1", sp_with(a=1.0)), ("a 0.5", sp_with(a=0.5)), ("thin 0", sp_with(thin=0))]
    fresh = buffers()
    untouched = state(fresh)
    for what, rc in [("null context", run(fresh, ctx=None)), ("null request", run(fresh, request=None)),
                     ("null fit spec", run(fresh, request=no_spec)), ("null stretch spec", run(fresh, sp=None)),
                     ("null pos", run(fresh, pos=1)), ("null lp", run(fresh, lp=1)), ("null accepted", run(fresh, acc=1)),
                     ("ndim of another fit", run(fresh, sp=sp_with(ndim=2))), ("n_steps < 0", run(fresh, n=-1))] + \
                    [(what, run(fresh, sp=s)) for what, s in bad_specs]:
        refused(rc, what)
    p = {k: v.data_ptr() for k, v in fresh.items()}
    for what, s in bad_specs + [("null", None)]:
        sp = ref(s) if s is not None else None
        refused(lib.vag_stretch_propose_dev(ctx, sp, 0, 0, p["pos"], p["prop"]), "propose: " + what)
        refused(lib.vag_stretch_accept_dev(ctx, sp, 0, 0, p["prop"], p["lp_new"], p["pos"], p["lp"], p["acc"]), "accept: " + what)
    for half in (-1, 2):
        assert "half" in refused(lib.vag_stretch_propose_dev(ctx, ref(good), 0, half, p["pos"], p["prop"]), "propose: half")
        assert "half" in refused(lib.vag_stretch_accept_dev(ctx, ref(good), 0, half, p["prop"], p["lp_new"], p["pos"], p["lp"], p["acc"]),
                                 "accept: half")
    refused(lib.vag_stretch_propose_dev(None, ref(good), 0, 0, p["pos"], p["prop"]), "propose: null context")
    refused(lib.vag_stretch_propose_dev(ctx, ref(good), 0, 0, None, p["prop"]), "propose: null pos")
    refused(lib.vag_stretch_propose_dev(ctx, ref(good), 0, 0, p["pos"], None), "propose: null prop")
    refused(lib.vag_stretch_accept_dev(None, ref(good), 0, 0, p["prop"], p["lp_new"], p["pos"], p["lp"], p["acc"]), "accept: null context")
    for k in range(5):
        args = [p["prop"], p["lp_new"], p["pos"], p["lp"], p["acc"]]
        args[k] = None
        refused(lib.vag_stretch_accept_dev(ctx, ref(good), 0, 0, *args), f"accept: null buffer {k}")
    assert run(fresh, n=0) == _lib.VAG_OK  # no step: nothing happens
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), untouched))
    # the context serves the valid call as before
    assert run(fresh) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), first))
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before
