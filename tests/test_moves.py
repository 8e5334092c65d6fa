"""The move mix of the device sampler (vag_move_propose_dev / _accept_dev / _run_dev; sampling.EnsembleMoves, run_moves_device,
fit(sampler="device", moves=...)) against its numpy statement (sampling.move_kind, de_proposals, snooker_proposals, move_accepts,
run_moves_philox).

Positions are compared with np.array_equal: the proposals are explicit fused operations, IEEE divisions and, for the DE move, a
normal quantised to 2^-20 whose distance from a rounding boundary is asserted (> 1e-9 of a quantum, against the ~1e-9 that the
rounding of log and cos can move n 2^20).  The decisions of the runs compared here are all further than 1e-9 from their thresholds
(asserted).  The ln of the Hastings factor goes only into the margin, never into a position, and carries one logarithm: both sides
take it of the same bits, each within 1 ulp, and multiply by h = (ndim - 1) / 2 (exact) with one rounding each, so the two factors
differ by at most 2 h ulp(L) + ulp(h L) <= 4 h ulp(L), L the logarithm -- the bound asserted (the stretch kind: h = ndim - 1).

1. proposals and factors of each kind over sizes, halves, steps beyond 2^32 and seeds beyond 2^32;
2. decisions and chain bits on the Gaussian of tests/test_sampler_host.py with the reference mix, ln p formed on the host;
3. vag_move_run_dev is the composition propose -> likelihood -> accept, whatever the chunk size; thinning; with the stretch move
   alone it is vag_stretch_run_dev's chain; the smallest ensembles; runs of the three entries of other sizes on one context;
4. proposals that are not finite, a snooker walker on its z;
5. Fitter.fit(sampler="device", moves="reference") end to end;
6. the refusals of the raw C-ABI, the context usable afterwards, device memory back after vag_ctx_destroy."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

import configs
import test_gpu_parity as tg
import test_sampler as ts
import test_sampler_host as sh
import test_sky_visfit as tv
import test_tempering as tt
from vegasafterglow_amd import _lib, fitting, sampling
from vegasafterglow_amd.fitting import _fma

pytestmark = pytest.mark.gpu

P = fitting.ParamDef
defs, TRUTH, start = ts.defs, ts.TRUTH, ts.start
torch, c4_data, c4 = ts.torch, ts.c4_data, ts.c4  # (the module-scoped fixtures of the stretch sampler's tests)
ONLY = {k: ((k, 1.0),) for k in sampling.MOVE_KINDS}
RUN_SEED = 7  # (the reference mix chooses DE, snooker, DE, snooker, DE, DE at steps 0..5 under this seed: asserted below)


def composed(torch, f, d, pos0, nsteps, seed, moves):
    """The run as a Python loop of the building blocks around Fitter.device_evaluator: (chain, logp, accepted counts, margins), the
    margins from sampling.move_accepts on what the device proposed and evaluated."""
    nw, ndim = pos0.shape
    move = sampling.EnsembleMoves(nw, ndim, moves=moves, seed=seed)
    eval_dev = f.device_evaluator(d, use_priors=True)
    pos = torch.from_numpy(pos0).cuda()
    lp = eval_dev(pos, want_costs=False)[0]
    accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
    chain, logp, margins = [], [], []
    nh = nw // 2
    for step in range(nsteps):
        for half in (0, 1):
            prop, factor = move.propose(step, half, pos)
            lp_new = eval_dev(prop, want_costs=False)[0]
            margins.append(sampling.move_accepts(step, half, seed, factor.cpu().numpy(), lp_new.cpu().numpy(),
                                                 lp.cpu().numpy()[half * nh:(half + 1) * nh])[1])
            move.accept(step, half, prop, factor, lp_new, pos, lp, accepted)
        chain.append(pos.cpu().numpy())
        logp.append(lp.cpu().numpy())
    return np.array(chain), np.array(logp), accepted.cpu().numpy(), np.concatenate(margins)


def snooker_log(pos, prop, partners, half):
    """L = log(|prop - z|^2 / |s - z|^2) of snooker_proposals, summed as there."""
    nh = pos.shape[0] // 2
    pz = pos[partners[:, 0]]
    delta, e = pos[half * nh:(half + 1) * nh] - pz, prop - pz
    r2, q2 = np.zeros(nh), np.zeros(nh)
    for d in range(pos.shape[1]):
        r2, q2 = _fma(delta[:, d], delta[:, d], r2), _fma(e[:, d], e[:, d], q2)
    return np.log(q2 / r2)


# ---------------------------------------------------------------- 1. proposals and factors
@pytest.mark.parametrize("nw,ndim", [(6, 1), (6, 3), (130, 3), (130, 16)])  # (130: the half of 65 straddles a wavefront)
def test_proposals_and_factors_are_the_host_statement(torch, nw, ndim):
    pos = np.random.default_rng(1).standard_normal((nw, ndim)) * np.logspace(-3, 3, ndim)
    d_pos = torch.from_numpy(pos).cuda()
    nh = nw // 2
    for seed in (0, 2 ** 40 + 7):
        moves = {k: sampling.EnsembleMoves(nw, ndim, moves=ONLY[k], seed=seed) for k in sampling.MOVE_KINDS}
        for step in (0, 1, 2 ** 32 + 5):
            for half in (0, 1):
                where = (nw, ndim, seed, step, half)
                # the stretch kind: vag_stretch_propose_dev's proposal, factor = (ndim - 1) log z
                got, got_f = (t.cpu().numpy() for t in moves["stretch"].propose(step, half, d_pos))
                want, z, _ = sampling.stretch_proposals(pos, step, half, seed)
                assert got.shape == (nh, ndim) and got_f.shape == (nh,)
                assert np.array_equal(got, want), where
                assert np.array_equal(got, sampling.StretchMove(nw, ndim, seed=seed).propose(step, half, d_pos).cpu().numpy()), where
                err, tol = np.abs(got_f - (ndim - 1.0) * np.log(z)), 4 * (ndim - 1.0) * np.spacing(np.abs(np.log(z)))
                print("stretch factor", where, "max err / tol", np.max(err / np.maximum(tol, 1e-300)))
                assert np.all(err <= tol), where
                # the DE kind: every row's normal is clear of a rounding boundary, so every row is compared
                got, got_f = (t.cpu().numpy() for t in moves["de"].propose(step, half, d_pos))
                want, want_f, partners, slack = sampling.de_proposals(pos, step, half, seed)
                assert np.all(slack > 1e-9), (where, slack.min())
                assert np.array_equal(got, want), (where, np.abs(got - want).max())
                assert np.array_equal(got_f, want_f) and np.all(got_f == 0.0)
                assert np.all(partners // nh == 1 - half) and np.all(partners[:, 0] != partners[:, 1])
                # the snooker kind
                got, got_f = (t.cpu().numpy() for t in moves["snooker"].propose(step, half, d_pos))
                want, want_f, partners = sampling.snooker_proposals(pos, step, half, seed)
                assert np.array_equal(got, want), (where, np.abs(got - want).max())
                assert np.all(np.isfinite(want_f)) and all(len(set(row)) == 3 for row in partners.tolist())
                err, tol = np.abs(got_f - want_f), 4 * (0.5 * (ndim - 1.0)) * np.spacing(np.abs(snooker_log(pos, want, partners, half)))
                print("snooker factor", where, "max err / tol", np.max(err / np.maximum(tol, 1e-300)))
                assert np.all(err <= tol), where
    assert np.array_equal(d_pos.cpu().numpy(), pos)  # proposing moves nothing


def test_other_scales_reach_the_kernels(torch):
    """gamma0, sigma, gamma_snooker and a are the spec's, not the defaults."""
    nw, ndim, seed = 10, 2, 4
    pos = np.random.default_rng(2).standard_normal((nw, ndim))
    d_pos = torch.from_numpy(pos).cuda()
    move = sampling.EnsembleMoves(nw, ndim, moves=ONLY["de"], seed=seed, gamma0=0.7, sigma=1e-2)
    want, _, _, slack = sampling.de_proposals(pos, 3, 1, seed, gamma0=0.7, sigma=1e-2)
    assert np.all(slack > 1e-9) and np.array_equal(move.propose(3, 1, d_pos)[0].cpu().numpy(), want)
    assert not np.array_equal(want, sampling.de_proposals(pos, 3, 1, seed)[0])
    move = sampling.EnsembleMoves(nw, ndim, moves=ONLY["snooker"], seed=seed, gamma_snooker=1.2)
    assert np.array_equal(move.propose(3, 1, d_pos)[0].cpu().numpy(), sampling.snooker_proposals(pos, 3, 1, seed, gamma_snooker=1.2)[0])
    move = sampling.EnsembleMoves(nw, ndim, moves=ONLY["stretch"], seed=seed, a=1.5)
    assert np.array_equal(move.propose(3, 1, d_pos)[0].cpu().numpy(), sampling.stretch_proposals(pos, 3, 1, seed, a=1.5)[0])


# ---------------------------------------------------------------- 2. decisions and chain bits
def test_decisions_and_chain_are_the_host_statement_to_the_bit(torch):
    nsteps, seed, pos0 = 300, sh.GAUSS_SEED, sh.gaussian_start()
    margins, slacks = [], []
    chain, logp, acc = sampling.run_moves_philox(sh.gaussian_log_prob, pos0, nsteps, moves=sampling.REFERENCE_MOVES, seed=seed,
                                                 margins=margins, slacks=slacks)
    assert np.abs(np.concatenate(margins)).min() > 1e-9 and np.concatenate(slacks).min() > 1e-9  # every decision and normal is compared
    nw, ndim = pos0.shape
    move = sampling.EnsembleMoves(nw, ndim, moves="reference", seed=seed)
    kinds = [move.kind(s) for s in range(nsteps)]
    assert set(kinds) == {1, 2} and 30 < kinds.count(2) < 90
    pos = torch.from_numpy(pos0).cuda()
    lp = torch.from_numpy(sh.gaussian_log_prob(pos0)).cuda()
    accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
    for step in range(nsteps):
        for half in (0, 1):
            prop, factor = move.propose(step, half, pos)
            lp_new = torch.from_numpy(sh.gaussian_log_prob(prop.cpu().numpy())).cuda()
            move.accept(step, half, prop, factor, lp_new, pos, lp, accepted)
        assert np.array_equal(pos.cpu().numpy(), chain[step]) and np.array_equal(lp.cpu().numpy(), logp[step]), (step, kinds[step])
    assert np.array_equal(accepted.cpu().numpy(), np.rint(acc * nsteps).astype(np.int64))
    assert 0.15 < acc.mean() < 0.6


# ---------------------------------------------------------------- 3. vag_move_run_dev is the composition
@pytest.fixture(scope="module")
def run130(torch, c4):
    d = defs()
    pos0, lo, hi = start(c4, d, 130, TRUTH)
    assert [sampling.move_kind(s, RUN_SEED, (0.0, 0.8, 0.2)) for s in range(6)] == [1, 2, 1, 2, 1, 1]
    return dict(d=d, pos0=pos0, lo=lo, hi=hi, run=sampling.run_moves_device(c4, d, pos0, 6, moves="reference", seed=RUN_SEED, chunk=6))


def test_run_is_the_composition_of_the_building_blocks(torch, c4, run130):
    chain, logp, acc = run130["run"]
    assert chain.shape == (6, 130, 3) and logp.shape == (6, 130) and acc.shape == (130,)
    want_chain, want_logp, want_count, _ = composed(torch, c4, run130["d"], run130["pos0"], 6, RUN_SEED, "reference")
    assert np.array_equal(chain, want_chain) and np.array_equal(logp, want_logp)
    assert np.array_equal(np.rint(acc * 6).astype(np.int64), want_count) and 0 < want_count.sum() < 6 * 130
    assert np.all(np.isfinite(logp)) and np.all(chain >= run130["lo"]) and np.all(chain <= run130["hi"])
    assert np.array_equal(logp[-1], c4.log_prob_batch(chain[-1], run130["d"]))  # positions and stored ln p belong together
    # every walker either stays or takes the proposal of the step's kind (the numpy statement on the device's chain)
    prev, nh = run130["pos0"], 65
    for step in range(6):
        mid = np.concatenate([chain[step][:nh], prev[nh:]])  # after the first half-step
        for half, before in ((0, prev), (1, mid)):
            s = slice(half * nh, half * nh + nh)
            prop, _, kind, slack = sampling.move_proposals(before, step, half, RUN_SEED, (0.0, 0.8, 0.2))
            assert kind == 2 or np.all(slack > 1e-9)
            stays, moves = np.all(chain[step][s] == before[s], axis=1), np.all(chain[step][s] == prop, axis=1)
            assert np.all(stays | moves) and moves.any(), (step, half)
        prev = chain[step]


@pytest.mark.parametrize("chunk", [4, 1])
def test_chunks_do_not_change_a_bit(c4, run130, chunk):
    seen = []
    got = sampling.run_moves_device(c4, run130["d"], run130["pos0"], 6, moves=sampling.REFERENCE_MOVES, seed=RUN_SEED, chunk=chunk,
                                    progress=lambda step, pos, lp: seen.append((step, pos.copy(), lp.copy())))
    assert all(np.array_equal(g, w) for g, w in zip(got, run130["run"]))
    assert [s for s, _, _ in seen] == ([3, 5] if chunk == 4 else list(range(6)))
    assert all(np.array_equal(pos, got[0][s]) and np.array_equal(lp, got[1][s]) for s, pos, lp in seen)


def test_thin_keeps_every_second_step(c4, run130):
    chain, logp, acc = sampling.run_moves_device(c4, run130["d"], run130["pos0"], 6, moves="reference", seed=RUN_SEED, thin=2, chunk=4)
    assert chain.shape == (3, 130, 3)
    assert np.array_equal(chain, run130["run"][0][1::2]) and np.array_equal(logp, run130["run"][1][1::2])
    assert np.array_equal(acc, run130["run"][2])


def test_stretch_alone_is_the_stretch_run(torch, c4, run130):
    """Weights (1, 0, 0): the chain of run_stretch_move_device, on a run none of whose decisions lies within 1e-9 of its threshold
    (the two entries round the margin differently: one adds a stored factor, the other may fuse the product into the sum)."""
    d, pos0 = run130["d"], run130["pos0"]
    _, _, _, margins = composed(torch, c4, d, pos0, 6, 5, ONLY["stretch"])
    assert np.abs(margins[np.isfinite(margins)]).min() > 1e-9
    want = sampling.run_stretch_move_device(c4, d, pos0, 6, seed=5, chunk=6)
    got = sampling.run_moves_device(c4, d, pos0, 6, moves=(("stretch", 1.0), ("de", 0.0), ("snooker", 0.0)), seed=5, chunk=4)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("kind,nw,free", [("snooker", 6, ("theta_c",)), ("de", 4, ("theta_c",)), ("de", 4, ("theta_c", "E_iso"))])
def test_smallest_ensembles_are_the_composition(torch, c4, kind, nw, free):
    """Halves of 3 for the snooker move and of 2 for the DE move: every walker of the other half is a partner."""
    by_name = {"theta_c": (P("theta_c", 0.02, 0.3), TRUTH[0]), "E_iso": (P("E_iso", 1e50, 1e54, fitting.Scale.log), TRUTH[2])}
    d = [by_name[n][0] for n in free] + tv._c4_fixed(skip=free)
    pos0, lo, hi = start(c4, d, nw, np.array([by_name[n][1] for n in free]))
    chain, logp, acc = sampling.run_moves_device(c4, d, pos0, 6, moves=ONLY[kind], seed=5, chunk=4)
    want_chain, want_logp, want_count, _ = composed(torch, c4, d, pos0, 6, 5, ONLY[kind])
    assert chain.shape == (6, nw, len(free))
    assert np.array_equal(chain, want_chain) and np.array_equal(logp, want_logp)
    assert np.array_equal(np.rint(acc * 6).astype(np.int64), want_count)
    assert np.array_equal(logp[-1], c4.log_prob_batch(chain[-1], d)) and np.all(chain >= lo) and np.all(chain <= hi)
    partners = (sampling.snooker_proposals if kind == "snooker" else sampling.de_proposals)(pos0, 0, 0, 5)[2]
    assert all(sorted(row) == list(range(nw // 2, nw)) for row in partners.tolist())


@contextlib.contextmanager
def fresh_context():
    """A new engine context in place of the process-wide one of device 0 (every call looks it up), destroyed on the way out."""
    from vegasafterglow_amd import model
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(h)))
    with model._ctx_lock:
        shared = model._ctx.pop(0, None)
        model._ctx[0] = (h, threading.RLock())
    try:
        yield
    finally:
        with model._ctx_lock:
            del model._ctx[0]
            if shared is not None:
                model._ctx[0] = shared
        lib.vag_ctx_destroy(h)


def test_the_three_run_entries_share_their_scratch_without_a_trace(c4):
    """One set of scratch buffers serves the three run entries, grown by whichever runs.  On one context, large, small, large: a
    ladder of 3 x 8 walkers, a stretch run of 130 (a half of 65 straddles a wavefront), the snooker move alone on 6 walkers with one
    free parameter (a half of 3), and the ladder again.  Every result is, array for array and bit for bit, that of the same call made
    first on a context of its own: no run reads what another left in the scratch or past its own part of it."""
    d3 = defs()
    d1 = [P("theta_c", 0.02, 0.3)] + tv._c4_fixed(skip=("theta_c",))
    ladder0, _, _ = tt.start(c4, d3, 3, 8, TRUTH)
    pos130, _, _ = start(c4, d3, 130, TRUTH)
    pos6, _, _ = start(c4, d1, 6, TRUTH[:1])
    runs = [lambda: sampling.run_tempered_device(c4, d3, ladder0, tt.BETAS3, 2, seed=5, priors=tt.PRIORS),
            lambda: sampling.run_stretch_move_device(c4, d3, pos130, 2, seed=5),
            lambda: sampling.run_moves_device(c4, d1, pos6, 2, moves=ONLY["snooker"], seed=5)]
    want = []
    for run in runs:
        with fresh_context():
            want.append(run())
    with fresh_context():
        got = [runs[k]() for k in (0, 1, 2, 0)]
    for g, w in zip(got, want + want[:1]):
        assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w))
    assert all(np.all(np.isfinite(a)) for g in got for a in g)


# ---------------------------------------------------------------- 4. what is not finite
@pytest.mark.parametrize("kind", sampling.MOVE_KINDS)
def test_a_proposal_that_is_not_finite_is_rejected(torch, kind):
    """NaN, +inf and -inf are rejected whatever the draw and the walker stays where it is; a huge finite ln p is taken."""
    nw, ndim = 8, 2
    move = sampling.EnsembleMoves(nw, ndim, moves=ONLY[kind], seed=9)
    pos0 = np.random.default_rng(3).standard_normal((nw, ndim))
    for half in (0, 1):
        pos = torch.from_numpy(pos0).cuda()
        lp = torch.zeros(nw, dtype=torch.float64, device=pos.device)
        accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
        prop, factor = move.propose(4, half, pos)
        assert bool(torch.isfinite(factor).all())
        lp_new = torch.tensor([np.nan, np.inf, -np.inf, 1e300], dtype=torch.float64, device=pos.device)
        move.accept(4, half, prop, factor, lp_new, pos, lp, accepted)
        s = slice(half * 4, half * 4 + 4)
        want_pos, want_lp = pos0.copy(), np.zeros(nw)
        want_pos[s][3], want_lp[s][3] = prop.cpu().numpy()[3], 1e300
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(lp.cpu().numpy(), want_lp)
        assert accepted.cpu().numpy()[s].tolist() == [0, 0, 0, 1] and accepted.cpu().numpy().sum() == 1


def test_a_snooker_walker_on_its_z_is_rejected(torch):
    """r2 = 0: the walker proposes its own position with factor -inf, and no ln p makes it move or count."""
    nw, ndim, seed, step = 12, 3, 11, 7
    pos0 = np.random.default_rng(5).standard_normal((nw, ndim))
    for half in (0, 1):
        partners = sampling.snooker_proposals(pos0, step, half, seed)[2]
        stuck = pos0.copy()
        w = half * 6 + 2
        stuck[w] = stuck[partners[2, 0]]
        want, want_f, _ = sampling.snooker_proposals(stuck, step, half, seed)
        assert want_f[2] == -np.inf and np.array_equal(want[2], stuck[w])
        move = sampling.EnsembleMoves(nw, ndim, moves=ONLY["snooker"], seed=seed)
        pos = torch.from_numpy(stuck).cuda()
        prop, factor = move.propose(step, half, pos)
        assert np.array_equal(prop.cpu().numpy(), want) and np.array_equal(np.isfinite(factor.cpu().numpy()), np.isfinite(want_f))
        assert factor.cpu().numpy()[2] == -np.inf
        lp = torch.zeros(nw, dtype=torch.float64, device=pos.device)
        accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
        lp_new = torch.full((6,), 1e300, dtype=torch.float64, device=pos.device)  # (every other walker takes its proposal)
        move.accept(step, half, prop, factor, lp_new, pos, lp, accepted)
        got_acc = accepted.cpu().numpy()
        assert got_acc[w] == 0 and got_acc.sum() == 5 and lp.cpu().numpy()[w] == 0.0
        assert np.array_equal(pos.cpu().numpy()[w], stuck[w])
        assert np.array_equal(np.delete(pos.cpu().numpy()[half * 6:half * 6 + 6], 2, axis=0), np.delete(want, 2, axis=0))


# ---------------------------------------------------------------- 5. end to end
def test_end_to_end_fit_with_the_reference_moves(oracle):
    """The assertions of test_end_to_end_fit_with_the_device_sampler on its problem, the proposals the reference's."""
    f, d = tg._c4_fitter(oracle)
    _, lo, hi = f.build_spec(d)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    ll_truth = f.loglike_batch(truth[None, :], d)[0]
    res = f.fit(d, nwalkers=32, nsteps=40, nburn=20, seed=1, sampler="device", moves="reference", center=truth + 0.05 * (hi - lo),
                spread=0.02)
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
    ref = C.byref

    def sp_with(**kw):
        s = _lib.MoveSpec(5, 2.0, 0.0, 1e-5, 1.7, (C.c_double * 3)(0.0, 0.8, 0.2), nw, ndim, 1)  # (gamma0 = 0: the default)
        for k, v in kw.items():
            setattr(s, k, (C.c_double * 3)(*v) if k == "weights" else v)
        return s

    good = sp_with()

    def buffers():
        b = dict(pos=torch.from_numpy(pos0).to(dev), lp=torch.from_numpy(lp0).to(dev),
                 acc=torch.zeros(nw, dtype=torch.int64, device=dev), chain=torch.zeros((nsteps, nw, ndim), dtype=torch.float64, device=dev),
                 logp=torch.zeros((nsteps, nw), dtype=torch.float64, device=dev), prop=torch.zeros((nw // 2, ndim), dtype=torch.float64, device=dev),
                 factor=torch.zeros(nw // 2, dtype=torch.float64, device=dev), lp_new=torch.zeros(nw // 2, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()  # (the context runs on a stream of its own)
        return b

    def run(b, ctx=ctx, request=request, sp=good, n=nsteps, **null):
        p = {k: (None if k in null else v.data_ptr()) for k, v in b.items()}
        rc = lib.vag_move_run_dev(ctx, ref(request) if request is not None else None, ref(sp) if sp is not None else None, 0, n,
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
    in_use = lib.vag_device_bytes_in_use()
    assert in_use > before

    def refused(rc, what):
        assert rc == _lib.VAG_E_INVALID, what
        msg = _lib.last_error()
        assert msg, what
        return msg

    nan, inf = float("nan"), float("inf")
    bad_specs = [("odd", sp_with(n_walkers=7)), ("few", sp_with(n_walkers=4)), ("ndim 0", sp_with(ndim=0)),
                 ("ndim 17", sp_with(ndim=17, n_walkers=40)), ("a nan", sp_with(a=nan)), ("a inf", sp_with(a=inf)), ("a 1", sp_with(a=1.0)),
                 ("thin 0", sp_with(thin=0)), ("weight < 0", sp_with(weights=(1.0, -0.1, 0.2))), ("weight nan", sp_with(weights=(nan, 0.8, 0.2))),
                 ("weight inf", sp_with(weights=(0.0, inf, 0.2))), ("weights all zero", sp_with(weights=(0.0, 0.0, 0.0))),
                 ("de with a half of 1", sp_with(n_walkers=2, ndim=1, weights=(0.0, 1.0, 0.0))),
                 ("snooker with a half of 2", sp_with(n_walkers=4, ndim=2, weights=(0.0, 0.8, 0.2))),
                 ("snooker with a half of 2, small weight", sp_with(n_walkers=4, ndim=1, weights=(1.0, 0.0, 1e-300))),
                 ("gamma0 < 0", sp_with(gamma0=-1.0)), ("gamma0 nan", sp_with(gamma0=nan)), ("gamma0 inf", sp_with(gamma0=inf)),
                 ("sigma nan", sp_with(sigma=nan)), ("sigma inf", sp_with(sigma=-inf)), ("gamma_snooker nan", sp_with(gamma_snooker=nan)),
                 ("gamma_snooker inf", sp_with(gamma_snooker=inf))]
    fresh = buffers()
    untouched = state(fresh)
    for what, rc in [("null context", run(fresh, ctx=None)), ("null request", run(fresh, request=None)),
                     ("null fit spec", run(fresh, request=_lib.LoglikeRequest())), ("null move spec", run(fresh, sp=None)),
                     ("null pos", run(fresh, pos=1)), ("null lp", run(fresh, lp=1)), ("null accepted", run(fresh, acc=1)),
                     ("chain without ln p", run(fresh, logp=1)), ("ln p without chain", run(fresh, chain=1)),
                     ("ndim of another fit", run(fresh, sp=sp_with(ndim=2))), ("n_steps < 0", run(fresh, n=-1))] + \
                    [(what, run(fresh, sp=s)) for what, s in bad_specs]:
        refused(rc, what)
        assert lib.vag_device_bytes_in_use() == in_use, what  # a refusal allocates nothing
    p = {k: v.data_ptr() for k, v in fresh.items()}
    for what, s in bad_specs + [("null", None)]:
        sp = ref(s) if s is not None else None
        refused(lib.vag_move_propose_dev(ctx, sp, 0, 0, p["pos"], p["prop"], p["factor"]), "propose: " + what)
        refused(lib.vag_move_accept_dev(ctx, sp, 0, 0, p["prop"], p["factor"], p["lp_new"], p["pos"], p["lp"], p["acc"]), "accept: " + what)
    for half in (-1, 2):
        assert "half" in refused(lib.vag_move_propose_dev(ctx, ref(good), 0, half, p["pos"], p["prop"], p["factor"]), "propose: half")
        assert "half" in refused(lib.vag_move_accept_dev(ctx, ref(good), 0, half, p["prop"], p["factor"], p["lp_new"], p["pos"], p["lp"],
                                                         p["acc"]), "accept: half")
    refused(lib.vag_move_propose_dev(None, ref(good), 0, 0, p["pos"], p["prop"], p["factor"]), "propose: null context")
    for k in range(3):
        args = [p["pos"], p["prop"], p["factor"]]
        args[k] = None
        refused(lib.vag_move_propose_dev(ctx, ref(good), 0, 0, *args), f"propose: null buffer {k}")
    refused(lib.vag_move_accept_dev(None, ref(good), 0, 0, p["prop"], p["factor"], p["lp_new"], p["pos"], p["lp"], p["acc"]), "accept: null context")
    for k in range(6):
        args = [p["prop"], p["factor"], p["lp_new"], p["pos"], p["lp"], p["acc"]]
        args[k] = None
        refused(lib.vag_move_accept_dev(ctx, ref(good), 0, 0, *args), f"accept: null buffer {k}")
    # what a weight of 0 does not ask for is not refused: DE alone on halves of 2, the stretch move alone on halves of 1
    assert lib.vag_move_propose_dev(ctx, ref(sp_with(n_walkers=4, ndim=2, weights=(0.0, 1.0, 0.0))), 0, 0, p["pos"], p["prop"], p["factor"]) == _lib.VAG_OK
    assert lib.vag_move_propose_dev(ctx, ref(sp_with(n_walkers=2, ndim=1, weights=(1.0, 0.0, 0.0))), 0, 0, p["pos"], p["prop"], p["factor"]) == _lib.VAG_OK
    _lib.check(lib.vag_ctx_synchronize(ctx))
    assert run(fresh, n=0) == _lib.VAG_OK  # no step: nothing happens
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), untouched))
    assert lib.vag_device_bytes_in_use() == in_use  # the account is where it was before the refused calls
    # the context serves the valid call as before
    assert run(fresh) == _lib.VAG_OK
    assert all(np.array_equal(u, v) for u, v in zip(state(fresh), first))
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before
