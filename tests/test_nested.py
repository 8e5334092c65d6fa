"""Nested sampling on the device (vag_nested_rank_dev / _retire_dev / _propose_dev / _accept_dev / _run_dev; sampling.NestedMove,
run_nested_device, fit(sampler="nested")) against its numpy statement (sampling.nested_order, nested_clones, nested_proposals,
nested_accepts, run_nested_philox).  Results are compared with np.array_equal: the ranks are integer counts, the proposals fused
operations on a quantised scale, the margins exact differences next to a logarithm, and the decisions compared here are all further
than 1e-9 from their thresholds (asserted), far above the rounding of a logarithm.

7. the building blocks to the bit over the shapes where the kernels take another path, ties in ln L included; the rank at N = 16384;
8. vag_nested_run_dev is the loop of the building blocks around vag_loglike_split_dev, whatever the chunk;
9. run_nested_device is run_nested_philox driven by the device's own ln L and ln prior;
10. the invariants of a real run;
11. Fitter.fit(sampler="nested") against the evidence and the posterior means of a grid that does not use the sampler;
12. the refusals of the raw C-ABI, the context usable afterwards, device memory back after vag_ctx_destroy."""
import ctypes as C
import math

import numpy as np
import pytest

import test_sky_visfit as tv
import test_tempering as tt
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu

P = fitting.ParamDef
defs, TRUTH, PRIORS = tt.defs, tt.TRUTH, tt.PRIORS
torch, c4_data, c4 = tt.torch, tt.c4_data, tt.c4  # (the module-scoped fixtures of tests/test_tempering.py)


def up(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------- 7. the building blocks
def tied_lnl(rng, n):
    """ln L with repeated values: quarter-integers in [-10, 0), so every value is shared by about n / 40 slots -- at n = 1024 within a
    256-slot tile and across tile boundaries -- and the point of rank n / 2 is given the value of rank n / 2 - 1 by hand, so that a tie
    sits on the boundary between the dead and the survivors."""
    lnl = rng.integers(-40, 0, n) / 4.0
    by_rank = np.argsort(lnl, kind="stable")
    lnl[by_rank[n // 2]] = lnl[by_rank[n // 2 - 1]]
    return lnl


# (4, 1): the smallest ensemble; (6, 2): K = 3, odd; (130, 3): K = 65 across a wavefront, N across a 256-lane group; (1024, 16): four
# LDS tiles in the rank kernel at the widest point
@pytest.mark.parametrize("n,ndim", [(4, 1), (6, 2), (130, 3), (1024, 16)])
def test_building_blocks_are_the_host_statement_to_the_bit(torch, n, ndim):
    rng = np.random.default_rng(n)
    k, walk = n // 2, 3
    live0 = rng.standard_normal((n, ndim)) * np.logspace(-3, 3, ndim)
    lnprior0 = rng.uniform(-3.0, -1.0, n)
    for seed in (0, 2 ** 40 + 7):
        for it in (0, 2 ** 32 + 5):
            lnl0 = tied_lnl(rng, n)
            move = sampling.NestedMove(n, ndim, walk, seed=seed)
            live, lnl, lnprior = up(torch, live0), up(torch, lnl0), up(torch, lnprior0)
            # rank
            order, lstar = move.rank(lnl)
            want_order, want_lstar = sampling.nested_order(lnl0)
            assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), want_order), (n, seed, it)
            assert lstar.cpu().numpy()[0] == want_lstar
            ranked = lnl0[want_order]
            assert (np.diff(ranked) == 0).sum() >= 1 and ranked[k - 1] == ranked[k]  # ties, one of them on the dead | survivor boundary
            assert np.array_equal(lnl.cpu().numpy(), lnl0)  # ranking moves nothing
            # retire
            dead = [torch.zeros((k,) + tail, dtype=torch.float64, device=live.device) for tail in ((ndim,), (), ())]
            move.retire(it, order, live, lnl, lnprior, *dead)
            src = sampling.nested_clones(want_order, it, walk, seed)
            slots = want_order[:k]
            assert set(src) <= set(want_order[k:])
            for got, before in zip(dead, (live0, lnl0, lnprior0)):
                assert np.array_equal(got.cpu().numpy(), before[slots])
            h_live, h_lnl, h_lnprior = live0.copy(), lnl0.copy(), lnprior0.copy()
            h_live[slots], h_lnl[slots], h_lnprior[slots] = live0[src], lnl0[src], lnprior0[src]
            assert np.array_equal(live.cpu().numpy(), h_live) and np.array_equal(lnl.cpu().numpy(), h_lnl)
            assert np.array_equal(lnprior.cpu().numpy(), h_lnprior)
            accepted = torch.zeros((k,), dtype=torch.int64, device=live.device)
            h_accepted = np.zeros(k, dtype=np.int64)
            for m in range(1, walk + 1):
                # proposals
                prop = move.propose(it, m, order, live)
                want, partners, slack = sampling.nested_proposals(h_live, want_order, it, m, walk, seed)
                assert slack.min() > 1e-9
                assert prop.shape == (k, ndim) and np.array_equal(prop.cpu().numpy(), want), (n, seed, it, m)
                assert np.all(partners[:, 0] != partners[:, 1]) and set(partners.ravel()) <= set(want_order[k:])
                # decisions: above, on and below L*, priors that rise and fall, and every kind of value that is not finite
                l_new = want_lstar + rng.uniform(-1.0, 3.0, k)
                p_new = h_lnprior[slots] + rng.uniform(-2.0, 1.0, k)
                l_new[0] = want_lstar  # on L*: rejected
                if k > 2:
                    l_new[1], p_new[2] = [np.nan, np.inf, -np.inf][m - 1], [np.nan, np.inf, -np.inf][m - 1]
                take, margin = sampling.nested_accepts(it, m, walk, seed, l_new, p_new, h_lnprior[slots], want_lstar)
                assert np.abs(margin[np.isfinite(margin)]).min(initial=1.0) > 1e-9 and not take[0]
                assert k <= 2 or (not take[1] and not take[2])
                move.accept(it, m, order, lstar, prop, up(torch, l_new), up(torch, p_new), live, lnl, lnprior, accepted)
                h_live[slots[take]], h_lnl[slots[take]], h_lnprior[slots[take]] = want[take], l_new[take], p_new[take]
                h_accepted += take
                assert np.array_equal(live.cpu().numpy(), h_live) and np.array_equal(lnl.cpu().numpy(), h_lnl), (n, seed, it, m)
                assert np.array_equal(lnprior.cpu().numpy(), h_lnprior) and np.array_equal(accepted.cpu().numpy(), h_accepted)
            assert n <= 6 or 0 < h_accepted.sum() < k * walk
            survivors = want_order[k:]
            assert np.array_equal(h_live[survivors], live0[survivors])  # the survivors did not move


def test_rank_at_the_largest_ensemble(torch):
    n = sampling.NESTED_MAX_LIVE
    lnl0 = tied_lnl(np.random.default_rng(5), n)
    move = sampling.NestedMove(n, 1, 1)
    order, lstar = move.rank(up(torch, lnl0))
    want_order, want_lstar = sampling.nested_order(lnl0)
    assert np.array_equal(order.cpu().numpy(), want_order) and lstar.cpu().numpy()[0] == want_lstar
    distinct = np.random.default_rng(6).permutation(n).astype(np.float64)  # no ties: the order is the inverse permutation
    order, lstar = move.rank(up(torch, distinct))
    assert np.array_equal(distinct[order.cpu().numpy()], np.arange(n)) and lstar.cpu().numpy()[0] == n // 2 - 1


# ---------------------------------------------------------------- 8. vag_nested_run_dev is the loop of the building blocks
N8, WALK8, ITERS8, SEED8 = 130, 4, 6, 5


def composed(torch, f, d, live0, niter, walk, seed, priors=None):
    """The run as a Python loop of the building blocks around vag_loglike_split_dev: a NestedRun."""
    n, ndim = live0.shape
    k = n // 2
    move = sampling.NestedMove(n, ndim, walk, seed=seed)
    spec, _, _ = f.build_spec(d, priors=priors, use_priors=True)
    live = torch.from_numpy(live0).cuda()
    dev = live.device
    lnl, lnprior = torch.empty((n,), dtype=torch.float64, device=dev), torch.empty((n,), dtype=torch.float64, device=dev)
    sampling.loglike_split_device(f, spec, live, lnl, lnprior)
    dead = [torch.zeros((niter, k) + tail, dtype=torch.float64, device=dev) for tail in ((ndim,), (), ())]
    accepted = torch.zeros((niter, k), dtype=torch.int64, device=dev)
    lnl_new, lnprior_new = torch.empty((k,), dtype=torch.float64, device=dev), torch.empty((k,), dtype=torch.float64, device=dev)
    for it in range(niter):
        order, lstar = move.rank(lnl)
        move.retire(it, order, live, lnl, lnprior, dead[0][it], dead[1][it], dead[2][it])
        for m in range(1, walk + 1):
            prop = move.propose(it, m, order, live)
            sampling.loglike_split_device(f, spec, prop, lnl_new, lnprior_new)
            move.accept(it, m, order, lstar, prop, lnl_new, lnprior_new, live, lnl, lnprior, accepted[it])
    return sampling.NestedRun(*[t.cpu().numpy() for t in dead], live.cpu().numpy(), lnl.cpu().numpy(), lnprior.cpu().numpy(),
                              accepted.cpu().numpy().sum(axis=1), niter, n + niter * k * walk)


def same_run(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def run130(torch, c4):
    d = defs()
    pos0, lo, hi = tt.start(c4, d, 1, N8, TRUTH)
    live0 = pos0[0]
    return dict(d=d, live0=live0, lo=lo, hi=hi,
                run=sampling.run_nested_device(c4, d, live0, ITERS8, walk=WALK8, seed=SEED8, chunk=ITERS8, priors=PRIORS))


def test_run_is_the_loop_of_the_building_blocks(torch, c4, run130):
    run = run130["run"]
    k = N8 // 2
    assert run.dead_theta.shape == (ITERS8, k, 3) and run.dead_lnl.shape == run.dead_lnprior.shape == (ITERS8, k)
    assert run.live.shape == (N8, 3) and run.lnl.shape == run.lnprior.shape == (N8,) and run.accepted.shape == (ITERS8,)
    want = composed(torch, c4, run130["d"], run130["live0"], ITERS8, WALK8, SEED8, priors=PRIORS)
    for name, got, w in zip(run._fields, run, want):
        assert np.array_equal(got, w), name
    assert np.all((run.accepted > 0) & (run.accepted < k * WALK8)) and run.niter == ITERS8
    assert np.ptp(run.lnprior) > 0  # the Gaussian prior of theta_v: the prior ratio does enter the decisions
    # positions and what is stored with them belong together
    again = c4.log_like_and_prior_batch(run.live, run130["d"], priors=PRIORS)
    assert np.array_equal(run.lnl, again[0]) and np.array_equal(run.lnprior, again[1])
    again = c4.log_like_and_prior_batch(run.dead_theta.reshape(-1, 3), run130["d"], priors=PRIORS)
    assert np.array_equal(run.dead_lnl.ravel(), again[0]) and np.array_equal(run.dead_lnprior.ravel(), again[1])


@pytest.mark.parametrize("chunk", [4, 1])
def test_chunks_do_not_change_a_bit_and_the_invariants_hold(c4, run130, chunk):
    """(10.) the flattened dead record is non-decreasing in ln L, every live ln L after iteration `it` is >= L* of that iteration, every
    stored value is finite, and ncall = N + iterations K walk."""
    seen = []
    got = sampling.run_nested_device(c4, run130["d"], run130["live0"], ITERS8, walk=WALK8, seed=SEED8, chunk=chunk, priors=PRIORS,
                                     progress=lambda it, live, lnl, lnprior: seen.append((it, live.copy(), lnl.copy(), lnprior.copy())))
    assert same_run(got, run130["run"])
    assert [s[0] for s in seen] == ([3, 5] if chunk == 4 else list(range(ITERS8)))
    assert np.array_equal(seen[-1][1], got.live) and np.array_equal(seen[-1][2], got.lnl) and np.array_equal(seen[-1][3], got.lnprior)
    assert np.all(np.diff(got.dead_lnl.ravel()) >= 0)
    for it, live, lnl, lnprior in seen:
        lstar = got.dead_lnl[it, -1]
        assert lnl.shape == (N8,) and np.all(lnl >= lstar) and (lnl > lstar).sum() >= N8 // 2  # the clones that never moved sit on a survivor
        assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnprior)) and np.all(np.isfinite(live))
        assert np.all(live >= run130["lo"]) and np.all(live <= run130["hi"])
    for arr in got[:6]:
        assert np.all(np.isfinite(arr))
    assert got.ncall == N8 + ITERS8 * (N8 // 2) * WALK8 and got.niter == ITERS8
    ev = sampling.nested_evidence(got.dead_lnl, got.lnl)
    assert np.isfinite(ev.ln_z) and ev.information > 0 and np.exp(ev.log_weights).sum() == pytest.approx(1.0, abs=1e-12)


# ---------------------------------------------------------------- 9. the device run against numpy
def test_device_run_is_the_numpy_statement_on_the_devices_own_likelihood(c4):
    """The smallest case: four live points, one free parameter, two walk steps, three iterations -- two proposals per likelihood call."""
    d = [P("theta_c", 0.02, 0.3)] + tv._c4_fixed(skip=("theta_c",))
    priors = {"theta_c": ("gaussian", 0.07, 0.01)}
    pos0, lo, hi = tt.start(c4, d, 1, 4, TRUTH[:1])
    margins, slacks = [], []
    want = sampling.run_nested_philox(lambda x: c4.log_like_and_prior_batch(x, d, priors=priors)[0],
                                      lambda x: c4.log_like_and_prior_batch(x, d, priors=priors)[1], pos0[0], 3, 2, seed=9, margins=margins,
                                      slacks=slacks)
    decided = np.concatenate(margins)
    assert np.abs(decided[np.isfinite(decided)]).min(initial=1.0) > 1e-9 and np.concatenate(slacks).min() > 1e-9
    got = sampling.run_nested_device(c4, d, pos0[0], 3, walk=2, seed=9, priors=priors)
    for name, g, w in zip(got._fields, got, want):
        assert np.array_equal(g, w), name
    assert got.dead_theta.shape == (3, 2, 1) and got.ncall == 4 + 3 * 2 * 2 and np.all(np.diff(got.dead_lnl.ravel()) >= 0)
    # a run under dlogz is the plain run of the iterations it ran
    stopped = sampling.run_nested_device(c4, d, pos0[0], 40, walk=2, seed=9, priors=priors, dlogz=0.5, chunk=2)
    assert 0 < stopped.niter < 40 and stopped.niter % 2 == 0
    assert sampling.nested_remaining(stopped.dead_lnl, stopped.lnl) < 0.5
    assert same_run(stopped, sampling.run_nested_device(c4, d, pos0[0], stopped.niter, walk=2, seed=9, priors=priors, chunk=3))
    if stopped.niter >= 3:
        assert np.array_equal(stopped.dead_lnl[:3], got.dead_lnl)


# ---------------------------------------------------------------- 11. end to end against a grid
# The box: log10 E_iso in [52.355, 52.445], theta_v in [0.3915, 0.4075], uniform priors.  With the other parameters at
# configs.C4_TRUTH the posterior of this data set has the means (52.4000, 0.39932) and the widths (0.0054, 0.00098), correlation 0.44:
# the box is 8 widths to either side.  On it the grid's ln Z is -30.33392 at 96 x 96 and -30.33393 at 64 x 64 (it moves by 1e-5), with
# H = 2.87 (measured on an MI355X; the test asserts the bound the comparison below allows for, 0.02).  The nested run there: 12
# iterations, ln Z = -30.45 +- 0.076, the Kish size of its weights 1446.
E_LO, E_HI, V_LO, V_HI = 52.355, 52.445, 0.3915, 0.4075
GRID_SHIFT = 0.02  # the bound asserted below on |ln Z(96 x 96) - ln Z(64 x 64)|


def defs11():
    return [P("E_iso", 10 ** E_LO, 10 ** E_HI, fitting.Scale.log), P("theta_v", V_LO, V_HI)] + tv._c4_fixed(skip=("E_iso", "theta_v"))


def grid_evidence(f, d, m):
    """ln Z, H and the posterior means and widths by the trapezoid rule over an m x m grid of the device likelihood, one batched call;
    the prior is uniform over the box, and points where the engine returns -inf count as L = 0."""
    e, v = np.linspace(E_LO, E_HI, m), np.linspace(V_LO, V_HI, m)
    pts = np.stack(np.meshgrid(e, v, indexing="ij"), axis=-1).reshape(-1, 2)
    lnl, lnprior = f.log_like_and_prior_batch(pts, d)
    assert np.all(np.isfinite(lnprior))
    lnl = np.where(np.isfinite(lnl), lnl, -np.inf).reshape(m, m)
    top = lnl.max()
    w1 = np.full(m, 1.0 / (m - 1))
    w1[[0, -1]] *= 0.5  # the trapezoid weights of the uniform prior density on [0, 1]
    w = np.outer(w1, w1) * np.exp(lnl - top)
    z = w.sum()
    p = w / z
    ln_z = top + math.log(z)
    h = float(np.sum(p * np.where(p > 0, lnl, 0.0)) - ln_z)
    mean = np.array([np.sum(p.sum(axis=1) * e), np.sum(p.sum(axis=0) * v)])
    sd = np.sqrt(np.array([np.sum(p.sum(axis=1) * (e - mean[0]) ** 2), np.sum(p.sum(axis=0) * (v - mean[1]) ** 2)]))
    return ln_z, h, mean, sd, float(np.mean(np.isfinite(lnl)))


def test_fit_nested_against_a_grid_evidence(c4):
    d = defs11()
    ln_z64, _, _, _, _ = grid_evidence(c4, d, 64)
    ln_z, h, mean, sd, finite = grid_evidence(c4, d, 96)
    print("grid: ln Z", ln_z, "at 64 x 64", ln_z64, "H", h, "means", mean, "widths", sd, "finite share", finite)
    assert abs(ln_z - ln_z64) < GRID_SHIFT
    assert np.all(mean - 3 * sd > [E_LO, V_LO]) and np.all(mean + 3 * sd < [E_HI, V_HI])  # a few posterior widths wide
    res = c4.fit(d, nwalkers=512, nsteps=200, seed=3, sampler="nested", dlogz=0.05)
    w = np.exp(res["log_weights"])
    ess = 1.0 / np.sum(w * w)
    got_mean = (w[:, None] * res["samples"]).sum(axis=0)
    print("nested: ln Z", res["log_evidence"], "+-", res["log_evidence_error"], "H", res["information"], "iterations", res["niter"],
          "ncall", res["ncall"], "prior fraction", res["prior_fraction"], "ESS", ess, "means", got_mean, "acceptance", res["acceptance"].mean())
    assert abs(res["log_evidence"] - ln_z) <= 5.0 * math.sqrt(h / 512) + GRID_SHIFT, (res["log_evidence"], ln_z)
    assert np.all(np.abs(got_mean - mean) <= 4.0 * sd / math.sqrt(ess)), (got_mean, mean, sd, ess)
    n_dead = res["niter"] * 256
    assert res["samples"].shape == (n_dead + 512, 2) and res["log_like"].shape == res["log_weights"].shape == (n_dead + 512,)
    assert res["equal_samples"].shape == res["samples"].shape and 0 < res["niter"] < 200
    assert np.all(np.diff(res["log_like"][:n_dead]) >= 0) and np.all(np.isfinite(res["log_like"]))
    assert np.all(res["samples"] >= [E_LO, V_LO]) and np.all(res["samples"] <= [E_HI, V_HI])
    assert res["log_prior_mass"] == 0.0 and 0 < res["prior_fraction"] <= 1.0 and res["prior_fraction"] == pytest.approx(finite, abs=0.05)
    tried = res["ncall"] - res["niter"] * 256 * sampling.nested_default_walk(2)  # the prior draws come in batches of nwalkers
    assert tried >= 512 and tried % 512 == 0 and res["prior_fraction"] * tried == pytest.approx(round(res["prior_fraction"] * tried), abs=1e-6)
    assert res["acceptance"].shape == (res["niter"],) and np.all((res["acceptance"] > 0) & (res["acceptance"] <= 1))
    assert res["log_evidence_error"] >= math.sqrt(res["information"] / 512) * (1 - 1e-12)
    assert np.array_equal(res["best"], res["samples"][np.argmax(res["log_like"] + res["log_prior"])])


# ---------------------------------------------------------------- 12. the raw C-ABI: refusals, the context afterwards, memory
def test_refusals_leave_the_context_usable_and_memory_returns(torch, c4):
    lib = _lib.load()
    d = defs()
    spec, _, _ = c4.build_spec(d, use_priors=True)
    request = fitting.loglike_request(spec)
    n, ndim, walk, niter = 8, 3, 2, 2
    k = n // 2
    pos0, _, _ = tt.start(c4, d, 1, n, TRUTH)
    lnl0, lnprior0 = c4.log_like_and_prior_batch(pos0[0], d)
    assert np.all(np.isfinite(lnl0)) and np.all(np.isfinite(lnprior0))
    dev = torch.device("cuda", 0)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def sp_with(**kw):
        s = _lib.NestedSpec(5, n, ndim, walk, 0, 0.0, 1e-5)
        for key, v in kw.items():
            setattr(s, key, v)
        return s

    good = sp_with()
    ref = C.byref
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731

    def buffers():
        b = dict(live=torch.from_numpy(pos0[0].copy()).to(dev), lnl=torch.from_numpy(lnl0).to(dev), lnprior=torch.from_numpy(lnprior0).to(dev),
                 acc=zeros(niter, k, dtype=torch.int64), dtheta=zeros(niter, k, ndim), dlnl=zeros(niter, k), dlnprior=zeros(niter, k),
                 order=zeros(n, dtype=torch.int32), lstar=zeros(1), prop=zeros(k, ndim), l_new=zeros(k), p_new=zeros(k))
        torch.cuda.synchronize()  # (the context runs on a stream of its own)
        return b

    RUN = ("live", "lnl", "lnprior", "acc", "dtheta", "dlnl", "dlnprior")

    def run(b, ctx=ctx, request=request, sp=good, it0=0, iters=niter, **null):
        p = {key: (None if key in null else v.data_ptr()) for key, v in b.items()}
        rc = lib.vag_nested_run_dev(ctx, ref(request) if request is not None else None, ref(sp) if sp is not None else None, it0, iters,
                                    *[p[key] for key in RUN])
        if ctx is not None:
            _lib.check(lib.vag_ctx_synchronize(ctx))
        return rc

    def state(b):
        return [b[key].cpu().numpy() for key in RUN]

    b = buffers()
    assert run(b) == _lib.VAG_OK
    first = state(b)
    # ... and it is the run of the Python driver
    want = sampling.run_nested_device(c4, d, pos0[0], niter, walk=walk, seed=5)
    assert np.array_equal(first[4], want.dead_theta) and np.array_equal(first[5], want.dead_lnl) and np.array_equal(first[6], want.dead_lnprior)
    assert np.array_equal(first[0], want.live) and np.array_equal(first[1], want.lnl) and np.array_equal(first[3].sum(axis=1), want.accepted)

    def refused(rc, what):
        assert rc == _lib.VAG_E_INVALID, what
        msg = _lib.last_error()
        assert msg, what
        return msg

    no_spec = _lib.LoglikeRequest()  # every block null
    bad_specs = [("odd", sp_with(n_live=7)), ("two", sp_with(n_live=2)), ("none", sp_with(n_live=0)), ("negative", sp_with(n_live=-4)),
                 ("too many", sp_with(n_live=16386)), ("ndim 0", sp_with(ndim=0)), ("ndim 17", sp_with(ndim=17)), ("walk 0", sp_with(walk=0)),
                 ("walk < 0", sp_with(walk=-1)), ("gamma0 nan", sp_with(gamma0=float("nan"))), ("gamma0 < 0", sp_with(gamma0=-1.0)),
                 ("gamma0 inf", sp_with(gamma0=float("inf"))), ("sigma nan", sp_with(sigma=float("nan"))), ("sigma inf", sp_with(sigma=float("inf")))]
    fresh = buffers()
    untouched = state(fresh)
    for what, rc in [("null context", run(fresh, ctx=None)), ("null request", run(fresh, request=None)),
                     ("null fit spec", run(fresh, request=no_spec)), ("null nested spec", run(fresh, sp=None)),
                     ("ndim of another fit", run(fresh, sp=sp_with(ndim=2))), ("n_iters < 0", run(fresh, iters=-1))] + \
                    [("null " + key, run(fresh, **{key: 1})) for key in RUN] + [(what, run(fresh, sp=s)) for what, s in bad_specs]:
        refused(rc, what)
    assert "live points" in refused(run(fresh, sp=sp_with(n_live=7)), "odd")
    p = {key: v.data_ptr() for key, v in fresh.items()}
    rank_args = [p["lnl"], p["order"], p["lstar"]]
    retire_args = [p["order"], p["live"], p["lnl"], p["lnprior"], p["dtheta"], p["dlnl"], p["dlnprior"]]
    propose_args = [p["order"], p["live"], p["prop"]]
    accept_args = [p["order"], p["lstar"], p["prop"], p["l_new"], p["p_new"], p["live"], p["lnl"], p["lnprior"], p["acc"]]
    for what, s in bad_specs + [("null", None)]:
        sp = ref(s) if s is not None else None
        refused(lib.vag_nested_rank_dev(ctx, sp, *rank_args), "rank: " + what)
        refused(lib.vag_nested_retire_dev(ctx, sp, 0, *retire_args), "retire: " + what)
        refused(lib.vag_nested_propose_dev(ctx, sp, 0, 1, *propose_args), "propose: " + what)
        refused(lib.vag_nested_accept_dev(ctx, sp, 0, 1, *accept_args), "accept: " + what)
    for m in (0, -1, walk + 1):
        assert "walk step" in refused(lib.vag_nested_propose_dev(ctx, ref(good), 0, m, *propose_args), "propose: m")
        assert "walk step" in refused(lib.vag_nested_accept_dev(ctx, ref(good), 0, m, *accept_args), "accept: m")
    refused(lib.vag_nested_rank_dev(None, ref(good), *rank_args), "rank: null context")
    refused(lib.vag_nested_retire_dev(None, ref(good), 0, *retire_args), "retire: null context")
    refused(lib.vag_nested_propose_dev(None, ref(good), 0, 1, *propose_args), "propose: null context")
    refused(lib.vag_nested_accept_dev(None, ref(good), 0, 1, *accept_args), "accept: null context")
    for entry, lead, args in ((lib.vag_nested_rank_dev, (), rank_args), (lib.vag_nested_retire_dev, (0,), retire_args),
                              (lib.vag_nested_propose_dev, (0, 1), propose_args), (lib.vag_nested_accept_dev, (0, 1), accept_args)):
        for i in range(len(args)):
            holed = list(args)
            holed[i] = None
            refused(entry(ctx, ref(good), *lead, *holed), f"{entry.__name__}: null buffer {i}")
    assert run(fresh, iters=0) == _lib.VAG_OK  # no iteration: nothing happens
    _lib.check(lib.vag_ctx_synchronize(ctx))
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), untouched))
    # the context serves the valid call as before, and a continuation from it0 repeats the single run
    assert run(fresh) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), first))
    parts = buffers()
    assert run(parts, iters=1) == _lib.VAG_OK
    tail = {key: (v[1:] if key in ("acc", "dtheta", "dlnl", "dlnprior") else v) for key, v in parts.items()}
    assert run(tail, it0=1, iters=1) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(parts), first))
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before
