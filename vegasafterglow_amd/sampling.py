"""Sampler-side glue for the batched device likelihood.

The reference drives emcee with ``vectorize=True`` and a ``log_prob_batch(samples[nb, ndim])`` closure that maps
walkers over a thread pool (VegasAfterglow/fitting/samplers.py:59-106).  Here the closure is one device call
(``Fitter.make_log_prob_batch``), so a sampler only has to hand over whole walker blocks:

* ``emcee_sampler``  -- the reference's own sampler object, wired to the device closure (needs emcee installed);
* ``run_stretch_move`` -- a dependency-free affine-invariant ensemble sampler (Goodman & Weare stretch move with the
  red-blue split emcee uses by default), so an end-to-end fit runs wherever the engine does.  Each half-step
  proposes nwalkers/2 walkers and evaluates them in ONE ``log_prob_batch`` call;
* ``run_stretch_move_device`` / ``StretchMove`` -- the stretch move itself on the device (fixed halves, Philox draws keyed by
  (seed, step, walker)): a run of steps is launches only, positions, ln p and the chain stay in HBM.  ``run_stretch_move_philox``,
  ``stretch_proposals`` and ``stretch_accepts`` state the same move in numpy, to the bit;
* ``run_moves_device`` / ``EnsembleMoves`` -- the same sampler with the reference's proposals: the differential-evolution move and
  the snooker move (``REFERENCE_MOVES``: DE at 0.8, snooker at 0.2), one kind per step chosen by weight, the stretch move among
  them.  ``run_moves_philox``, ``move_kind``, ``de_proposals``, ``snooker_proposals`` and ``move_accepts`` state them in numpy;
* ``run_tempered_device`` / ``TemperedMove`` -- parallel tempering around that move on the device: a ladder of inverse temperatures
  (``geometric_betas``), all temperatures' proposals in one likelihood call per half-step, exchanges between neighbours, and the
  evidence by thermodynamic integration (``thermodynamic_evidence``).  ``run_tempered_philox``, ``tempered_proposals``,
  ``tempered_accepts`` and ``tempered_swaps`` state it in numpy, to the bit;
* ``run_nested_device`` / ``NestedMove`` -- nested sampling on the device: every iteration retires the lower half of the live points
  and replaces each by a clone of a survivor that walks constrained DE steps, the half's proposals in one likelihood call per walk
  step; the evidence and its error come out of the run (``nested_evidence``).  ``run_nested_philox``, ``nested_order``,
  ``nested_clones``, ``nested_proposals`` and ``nested_accepts`` state it in numpy, to the bit; ``sample_prior`` and ``prior_mass``
  draw from and integrate the priors the device evaluates;
* ``chain_autocorr_device`` / ``Convergence`` -- the integrated autocorrelation time of every parameter of a chain that lives on the
  device (pooled over the walkers, Sokal's window), and the stopping rule built on it: ``converge=`` makes ``nsteps`` of the three
  device run drivers a maximum.  ``chain_autocorr``, ``chain_mean`` and ``sokal_window`` state the estimate in numpy;
* ``column_quantiles_device`` -- the quantiles of every column of an array of draws that lives on the device, over its valid draws:
  the stage behind ``Fitter.predict``'s posterior-predictive bands.  ``column_quantiles`` states it in numpy, to the bit;
* ``BatchPool`` -- the object handed to ``bilby.run_sampler(pool=...)`` in place of the reference's thread pool
  (samplers.py:146-170): ``pool.map(loglikelihood, points)`` becomes one device call over the whole live-point queue.
"""
import math
from collections import namedtuple
from typing import Callable, Optional, Sequence

import numpy as np

from .fitting import Fitter, ParamDef


def initial_positions(lower: np.ndarray, upper: np.ndarray, nwalkers: int, rng: np.random.Generator,
                      center: Optional[np.ndarray] = None, spread: float = 0.1) -> np.ndarray:
    """Walkers in a ball of relative width `spread` (of the box) around `center` (default: the box centre), clipped
    to the bounds -- the strategy of generate_initial_positions (fitting/samplers.py) for uniform priors."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    c = 0.5 * (lower + upper) if center is None else np.asarray(center, dtype=np.float64)
    pos = c + spread * (upper - lower) * rng.standard_normal((nwalkers, lower.size))
    eps = 1e-9 * (upper - lower)
    return np.clip(pos, lower + eps, upper - eps)


def emcee_sampler(fitter: Fitter, param_defs: Sequence[ParamDef], nwalkers: int, loglike_fn: Optional[Callable] = None,
                  moves=None):
    """emcee.EnsembleSampler(nwalkers, ndim, log_prob_batch, vectorize=True, moves=moves) exactly like
    fitting/samplers.py:109-115, with the device closure in place of the thread-pool one."""
    import emcee  # optional dependency, as in the reference

    log_prob_batch = fitter.make_log_prob_batch(param_defs, loglike_fn=loglike_fn)
    spec, _, _ = fitter.build_spec(param_defs)
    return emcee.EnsembleSampler(nwalkers, spec.ndim, log_prob_batch, vectorize=True, moves=moves)


class BatchPool:
    """Drop-in for ThreadPoolWithClose (fitting/samplers.py:146-170) as bilby / dynesty use it: with
    ``use_pool={"loglikelihood": True}`` the sampler calls ``pool.map(loglikelihood, queue)`` with ``queue_size`` points
    in sampler space; here the whole queue goes through ``batch_fn(points[n, ndim]) -> float64[n]`` (one device call,
    e.g. ``fitter.make_log_prob_batch(defs)`` or ``lambda v: fitter.loglike_batch(v, defs)``) and the per-point callable
    is only used for anything that is not a point queue."""

    def __init__(self, batch_fn: Callable[[np.ndarray], np.ndarray], ndim: int, size: int = 1024):
        self.batch_fn, self.ndim, self.size = batch_fn, int(ndim), int(size)  # `size`: queue length dynesty should fill
        self.calls = 0

    def map(self, func, iterable, chunksize=None):
        tasks = list(iterable)
        if not tasks:
            return []
        try:
            pts = np.asarray(tasks, dtype=np.float64)
        except (TypeError, ValueError):
            pts = None
        if pts is None or pts.ndim != 2 or pts.shape[1] != self.ndim:
            return [func(x) for x in tasks]
        self.calls += 1
        out = np.asarray(self.batch_fn(pts), dtype=np.float64)
        out[~np.isfinite(out)] = -np.inf  # non-finite likelihoods are rejected points (samplers.py:66-70)
        return list(out)

    def close(self):
        pass

    def join(self):
        pass

    def shutdown(self, wait=True):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def run_stretch_move(log_prob_batch: Callable[[np.ndarray], np.ndarray], pos0: np.ndarray, nsteps: int,
                     rng: Optional[np.random.Generator] = None, a: float = 2.0, progress: Optional[Callable] = None):
    """Affine-invariant ensemble MCMC (Goodman & Weare 2010, stretch move, red-blue halves).

    Returns (chain[nsteps, nwalkers, ndim], log_prob[nsteps, nwalkers], acceptance_fraction[nwalkers]).
    `log_prob_batch` is called twice per step with nwalkers/2 rows each."""
    rng = np.random.default_rng() if rng is None else rng
    pos = np.array(pos0, dtype=np.float64, copy=True)
    nwalkers, ndim = pos.shape
    if nwalkers < 2 * ndim or nwalkers % 2:
        raise ValueError("need an even number of walkers, at least 2 * ndim")
    lp = np.asarray(log_prob_batch(pos), dtype=np.float64)
    if not np.all(np.isfinite(lp)):
        raise ValueError("initial positions must have finite log-probability")
    chain = np.empty((nsteps, nwalkers, ndim))
    logp = np.empty((nsteps, nwalkers))
    accepted = np.zeros(nwalkers)
    half = nwalkers // 2
    idx = np.arange(nwalkers)
    for step in range(nsteps):
        perm = rng.permutation(nwalkers)
        for first in (True, False):
            s = perm[:half] if first else perm[half:]  # walkers being updated
            c = perm[half:] if first else perm[:half]  # the complementary ensemble
            z = ((a - 1.0) * rng.random(half) + 1.0) ** 2 / a  # g(z) ~ 1/sqrt(z) on [1/a, a]
            partner = pos[c[rng.integers(half, size=half)]]
            prop = partner + z[:, None] * (pos[s] - partner)
            lp_new = np.asarray(log_prob_batch(prop), dtype=np.float64)
            lp_new[~np.isfinite(lp_new)] = -np.inf
            log_ratio = (ndim - 1.0) * np.log(z) + lp_new - lp[s]
            take = np.log(rng.random(half)) < log_ratio
            pos[s[take]] = prop[take]
            lp[s[take]] = lp_new[take]
            accepted[s[take]] += 1
        chain[step], logp[step] = pos, lp
        if progress is not None:
            progress(step, pos, lp)
    del idx
    return chain, logp, accepted / max(nsteps, 1)


# ---- the stretch move with fixed halves and counter-based draws: the host statement of the device sampler (INTEGRATION.md
#      "The device sampler").  A chain is a pure function of (seed, step, walker) and of ln p. ----

_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al. 2011, the Random123 constants), vectorised: counter[..., 4] and key[..., 2] of 32-bit words
    (broadcast against each other) -> uint32[..., 4]."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., i] & _MASK32, shape) for i in range(4)]
    k = [np.broadcast_to(key[..., i] & _MASK32, shape) for i in range(2)]
    s32 = np.uint64(32)
    for r in range(10):
        k0 = (k[0] + np.uint64((r * _PHILOX_W0) & 0xFFFFFFFF)) & _MASK32
        k1 = (k[1] + np.uint64((r * _PHILOX_W1) & 0xFFFFFFFF)) & _MASK32
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]  # (32 x 32 bits: exact in 64)
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> s32) ^ c[3] ^ k1, p0 & _MASK32]
    return np.stack(c, axis=-1).astype(np.uint32)


def _u53(hi, lo):
    """The uniform in [0, 1) of two Philox words: ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, exact in a double."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    return (((hi >> np.uint64(5)) << np.uint64(26)) + (lo >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def _stretch_words(nwalkers, step, half, seed, stream):
    """The four Philox words of every walker of half `half` (0: walkers [0, nwalkers / 2), 1: the rest) at absolute step `step`."""
    nh = nwalkers // 2
    step, seed = int(step), int(seed)
    counter = np.empty((nh, 4), dtype=np.uint64)
    counter[:, 0] = half * nh + np.arange(nh)
    counter[:, 1], counter[:, 2], counter[:, 3] = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, stream
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))


def _check_stretch(nwalkers, ndim, a=2.0, thin=1):
    if nwalkers % 2 or nwalkers < 2 * ndim:
        raise ValueError("need an even number of walkers, at least 2 * ndim")
    if not 1 <= ndim <= 16:
        raise ValueError("the stretch move takes 1..16 dimensions")
    if not (np.isfinite(a) and a > 1.0):
        raise ValueError("the stretch scale a must be finite and > 1")
    if thin < 1:
        raise ValueError("thin must be >= 1")


def stretch_z(a, u):
    """vag::stretch_z in numpy: z = t t / a with t = fma(a - 1, u, 1), g(z) ~ 1 / sqrt(z) on [1 / a, a).  The half-open end is kept
    in floating point: for the last few u below 1 the fma rounds t up to a, and z is then the largest double below a."""
    from .fitting import _fma
    t = _fma(a - 1.0, u, 1.0)
    z = t * t / a
    return np.where(z < a, z, np.nextafter(a, 0.0))


def stretch_proposals(pos, step, half, seed, a=2.0):
    """The proposals of half `half` (0 or 1) at absolute step `step`: (prop[nw / 2, ndim], z[nw / 2], partner[nw / 2]), partner the
    index in the whole ensemble of the walker of the other half each one stretches from.  Bit for bit what
    vag_stretch_propose_dev computes (fitting._fma for its two fused operations)."""
    from .fitting import _fma
    pos = np.asarray(pos, dtype=np.float64)
    nw = pos.shape[0]
    nh = nw // 2
    x = _stretch_words(nw, step, half, seed, 0)
    z = stretch_z(a, _u53(x[:, 0], x[:, 1]))
    partner = (1 - half) * nh + ((x[:, 2].astype(np.uint64) * np.uint64(nh)) >> np.uint64(32)).astype(np.int64)
    other = pos[partner]
    return _fma(z[:, None], pos[half * nh:(half + 1) * nh] - other, other), z, partner


def stretch_accepts(step, half, seed, z, lp_new, lp_old, ndim):
    """The decisions of half `half` at step `step`: (take[nw / 2], margin[nw / 2]).  A proposal whose ln p is not finite is rejected
    (margin -inf); any other is taken iff log(u_a) < (ndim - 1) log z + (lp_new - lp_old), and margin is that right side minus the
    left: a decision whose |margin| is far above the rounding of the logarithms is the same on every machine."""
    z, lp_new, lp_old = (np.asarray(v, dtype=np.float64) for v in (z, lp_new, lp_old))
    y = _stretch_words(2 * z.size, step, half, seed, 1)
    finite = np.isfinite(lp_new)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = ((ndim - 1.0) * np.log(z) + (lp_new - lp_old)) - np.log(_u53(y[:, 0], y[:, 1]))  # (u_a = 0: log = -inf, taken)
    margin = np.where(finite, margin, -np.inf)
    return finite & (margin > 0), margin


def run_stretch_move_philox(log_prob_batch: Callable[[np.ndarray], np.ndarray], pos0: np.ndarray, nsteps: int, seed: int = 0,
                            a: float = 2.0, thin: int = 1, step0: int = 0, margins: Optional[list] = None):
    """The chain of the device sampler through any host callable: the stretch move with fixed halves (half 0 = walkers
    [0, nw / 2) against half 1, then half 1 against the updated half 0, no permutation) and Philox draws keyed by (seed, step,
    walker).  Runs steps step0 .. step0 + nsteps - 1 and stores step s when (s + 1) % thin == 0.

    Returns (chain[rows, nw, ndim], log_prob[rows, nw], acceptance[nw]).  ``margins``: a list that receives every half-step's
    margin array (stretch_accepts)."""
    pos = np.array(pos0, dtype=np.float64, copy=True)
    nw, ndim = pos.shape
    _check_stretch(nw, ndim, a, thin)
    lp = np.asarray(log_prob_batch(pos), dtype=np.float64).copy()
    if not np.all(np.isfinite(lp)):
        raise ValueError("initial positions must have finite log-probability")
    rows = (step0 + nsteps) // thin - step0 // thin
    chain, logp = np.empty((rows, nw, ndim)), np.empty((rows, nw))
    accepted = np.zeros(nw, dtype=np.int64)
    nh, row = nw // 2, 0
    for step in range(step0, step0 + nsteps):
        for half in (0, 1):
            s = slice(half * nh, (half + 1) * nh)
            prop, z, _ = stretch_proposals(pos, step, half, seed, a)
            lp_new = np.asarray(log_prob_batch(prop), dtype=np.float64)
            take, margin = stretch_accepts(step, half, seed, z, lp_new, lp[s], ndim)
            if margins is not None:
                margins.append(margin)
            pos[s][take] = prop[take]
            lp[s][take] = lp_new[take]
            accepted[s][take] += 1
        if (step + 1) % thin == 0:
            chain[row], logp[row] = pos, lp
            row += 1
    return chain, logp, accepted / max(nsteps, 1)


class _DeviceMove:
    """What StretchMove, EnsembleMoves, TemperedMove and NestedMove share: the library, the device's context with its lock, the spec struct, the
    entry points (lookup(lib, name), kept as self._<key>), the check of a tensor argument and the call of an entry point."""

    def __init__(self, lookup, spec, device, **entries):
        import torch
        from . import _lib
        from .model import get_context
        self._lib = _lib.load()
        for key, name in entries.items():
            setattr(self, "_" + key, lookup(self._lib, name))
        self._spec = spec
        self._h, self._lock = get_context(device)
        self._dev = torch.device("cuda", device)

    def _checked(self, t, shape, dtype, what):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != self._dev or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {shape} on {self._dev}")
        return t

    def _call(self, entry, *args):
        """entry(context, spec, *args) on torch's current stream, a tensor among args as its data pointer."""
        import ctypes as C
        from . import _lib
        from .fitting import on_current_stream
        args = [a.data_ptr() if hasattr(a, "data_ptr") else int(a) for a in args]
        on_current_stream(self._lib, self._h, self._lock, self._dev, lambda: _lib.check(entry(self._h, C.byref(self._spec), *args)))


class StretchMove(_DeviceMove):
    """The two halves of a half-step on the device (vag_stretch_propose_dev / vag_stretch_accept_dev), on float64 torch tensors and
    torch's current stream; nothing crosses PCIe and nothing synchronises.  They need no model: any evaluator on device tensors goes
    between them, a dist.WalkerSharder for instance::

        move = StretchMove(nw, ndim, seed=7)
        lp, _ = eval_dev(pos)                                # ln p of the whole ensemble, float64[nw] on the device
        accepted = torch.zeros(nw, dtype=torch.int64, device=pos.device)
        for step in range(nsteps):
            for half in (0, 1):
                prop = move.propose(step, half, pos)         # [nw / 2, ndim]
                lp_new = sharder.log_prob(prop)              # or eval_dev(prop)[0]: any float64[nw / 2] on the device
                move.accept(step, half, prop, lp_new, pos, lp, accepted)   # pos, lp, accepted change in place

    The chain is the one sampling.run_stretch_move_philox makes from the same ln p."""

    def __init__(self, nwalkers: int, ndim: int, seed: int = 0, a: float = 2.0, device: int = 0):
        _check_stretch(nwalkers, ndim, a)
        from . import _lib
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        super().__init__(_lib.stretch_entry, _lib.StretchSpec(int(seed) & (2 ** 64 - 1), float(a), self.nwalkers, self.ndim, 1), device,
                         propose="vag_stretch_propose_dev", accept="vag_stretch_accept_dev")

    def propose(self, step: int, half: int, pos):
        import torch
        self._checked(pos, (self.nwalkers, self.ndim), torch.float64, "pos")
        prop = torch.empty((self.nwalkers // 2, self.ndim), dtype=torch.float64, device=self._dev)
        self._call(self._propose, step, half, pos, prop)
        return prop

    def accept(self, step: int, half: int, prop, lp_new, pos, lp, accepted):
        import torch
        nh = self.nwalkers // 2
        self._checked(prop, (nh, self.ndim), torch.float64, "prop")
        self._checked(lp_new, (nh,), torch.float64, "lp_new")
        self._checked(pos, (self.nwalkers, self.ndim), torch.float64, "pos")
        self._checked(lp, (self.nwalkers,), torch.float64, "lp")
        self._checked(accepted, (self.nwalkers,), torch.int64, "accepted")
        self._call(self._accept, step, half, prop, lp_new, pos, lp, accepted)


def _run_chunks(fitter: Fitter, param_defs, priors, who, pos0_text, ndim, proposals, nsteps, thin, chunk, progress, converge, nburn, record,
                cold, entry, move, begin, stop=None):
    """The chunk driver behind run_stretch_move_device, run_moves_device, run_tempered_device and run_nested_device.  The caller has checked pos0
    (pos0_text: what it says of a pos0 of another ndim than the fit's) and made `move`, the struct the run entry `entry(lib)` takes
    behind the request.  begin(lib, h, lock, dev, spec, rows) allocates and returns (state, counts, chains): the tensors of the
    current state, positions first, evaluated and found finite; the count tensors; the tensors of `rows` stored rows, the chain
    first -- each list in the order of the run entry's arguments.  cold(chain): the view [rows, W, D] the convergence monitor reads;
    proposals: those of one likelihood call, for the plan's warnings.  ``progress(step, *state)`` gets numpy copies once per chunk.

    stop(state, chains, ran), if given, is asked after every chunk and ends the run where it returns True (nested sampling's dlogz).

    Returns (chains, counts, ran, rec, state) as numpy arrays: the rows of the `ran` steps run, the counts, the ConvergedAutocorr
    record -- None for a plain run (converge=None and no `record`), which runs all its steps -- and the state the run left."""
    import ctypes as C
    import torch
    from . import _lib
    from .fitting import loglike_request, on_current_stream
    from .model import get_context
    if chunk < 1 or nsteps < 0:
        raise ValueError("chunk must be >= 1 and nsteps >= 0")
    monitor = _ConvergenceMonitor(converge, nsteps, nburn, thin, chunk, fitter.device, cold)
    spec, _, _ = fitter.build_spec(param_defs, priors=priors, use_priors=True)
    if spec.ndim != ndim:
        raise ValueError(pos0_text)
    fitter._refuse_host_priors(param_defs, who)
    lib = _lib.load()
    run = entry(lib)
    h, lock = get_context(fitter.device)
    dev = torch.device("cuda", fitter.device)
    request = loglike_request(spec)
    rows = nsteps // thin
    state, counts, chains = begin(lib, h, lock, dev, spec, rows)
    step0 = 0
    while step0 < nsteps:
        n = monitor.chunk_end(step0) - step0
        row = step0 // thin
        at = [c[row].data_ptr() if row < rows else None for c in chains]  # (a chunk of no stored row stores nothing)
        on_current_stream(lib, h, lock, dev, lambda: _lib.check(run(h, C.byref(request), C.byref(move), step0, n,
                                                                    *[t.data_ptr() for t in state + counts], *at)))
        if progress is not None:
            progress(step0 + n - 1, *[t.cpu().numpy() for t in state])
        step0 += n
        if monitor.stop(chains[0], step0) or (stop is not None and stop(state, chains, step0)):
            break
    plan = _lib.Plan()
    with lock:
        lib.vag_last_plan(h, C.byref(plan))
    fitter._log_plan_warnings(plan, proposals)
    fitter.last_plan = plan
    plain = converge is None and not record
    kept = step0 // thin  # (step0: the steps run; a plain run has run nsteps)
    return ([c[:kept].cpu().numpy() for c in chains], [t.cpu().numpy() for t in counts], step0,
            None if plain else monitor.record(chains[0], step0), [t.cpu().numpy() for t in state])


def _run_halves_device(fitter: Fitter, param_defs, pos0, nsteps, thin, priors, chunk, progress, who, entry, make_move, converge=None,
                       nburn=0, _record=False):
    """The body of run_stretch_move_device and run_moves_device: `entry` is the run entry's name and make_move(nw, ndim) the
    struct it takes behind the request (after the Python-side checks, which make_move performs).  converge, nburn: the stopping
    rule (_ConvergenceMonitor); with converge=None the loop is the plain one, chunk by chunk."""
    from . import _lib
    pos0 = np.ascontiguousarray(pos0, dtype=np.float64)
    if pos0.ndim != 2:
        raise ValueError("pos0 must be [nwalkers, ndim]")
    nw, ndim = pos0.shape
    move = make_move(nw, ndim)

    def begin(lib, h, lock, dev, spec, rows):
        import ctypes as C
        import torch
        from .fitting import _widest_entry, on_current_stream
        pos = torch.from_numpy(pos0).to(dev)
        lp = torch.empty((nw,), dtype=torch.float64, device=dev)
        accepted = torch.zeros((nw,), dtype=torch.int64, device=dev)
        chain = torch.empty((rows, nw, ndim), dtype=torch.float64, device=dev)
        logp = torch.empty((rows, nw), dtype=torch.float64, device=dev)
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731

        def initial():
            fn, fold = _widest_entry(lib, spec, "_dev")
            _lib.check(fn(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise),
                          ref(spec._counts), ref(spec._index), *fold, pos.data_ptr(), nw, ndim, lp.data_ptr()))
        on_current_stream(lib, h, lock, dev, initial)
        if not bool(torch.isfinite(lp).all()):
            raise ValueError("initial positions must have finite log-probability")
        return [pos, lp], [accepted], [chain, logp]
    lookup = _lib.stretch_entry if entry == "vag_stretch_run_dev" else _lib.move_entry
    (chain, logp), (accepted,), ran, rec, _ = _run_chunks(fitter, param_defs, priors, who, "pos0 must be [nwalkers, ndim]", ndim, nw // 2, nsteps,
                                                       thin, chunk, progress, converge, nburn, _record, lambda kept: kept,
                                                       lambda lib: lookup(lib, entry), move, begin)
    out = (chain, logp, accepted / max(ran, 1))
    return out if rec is None else out + (rec,)


def run_stretch_move_device(fitter: Fitter, param_defs: Sequence[ParamDef], pos0: np.ndarray, nsteps: int, seed: int = 0,
                            a: float = 2.0, thin: int = 1, priors=None, chunk: int = 64, progress: Optional[Callable] = None,
                            converge: Optional["Convergence"] = None, nburn: int = 0, _record: bool = False):
    """The stretch move of run_stretch_move_philox with everything on the device: the spec is built once, and every `chunk` steps are
    ONE call (vag_stretch_run_dev) that scans and uploads the spec blocks once and then only launches -- positions, ln p, the chain
    and the acceptance counts stay in HBM, nothing is copied and the stream is not synchronised between steps.  ln p is
    ln L + sum ln prior with the bounds mask (Fitter.log_prob_batch); only priors that run on the device are accepted.

    Returns (chain[nsteps // thin, nw, ndim], log_prob[nsteps // thin, nw], acceptance[nw]) as numpy arrays.  The chunk size does
    not change a bit of them.  ``progress(step, pos, lp)`` is called once per chunk with the last step of the chunk; the context's
    lock is free between chunks.

    ``converge=Convergence(...)`` makes ``nsteps`` a maximum: the chunks are clipped so that a check lands after every
    ``converge.check`` steps, where the autocorrelation times of the stored rows from ``nburn // thin`` on are estimated on the device
    (chain_autocorr_device: only tau and the windows come to the host), and the run stops at the first check that meets the rule
    (Convergence).  The three arrays are then those of a plain run of the steps run, to the bit, and a fourth element follows: the
    ConvergedAutocorr record.  With ``converge=None`` nothing changes."""
    def make_move(nw, ndim):
        from . import _lib
        _check_stretch(nw, ndim, a, thin)
        return _lib.StretchSpec(int(seed) & (2 ** 64 - 1), float(a), nw, ndim, int(thin))
    return _run_halves_device(fitter, param_defs, pos0, nsteps, thin, priors, chunk, progress, "run_stretch_move_device",
                              "vag_stretch_run_dev", make_move, converge, nburn, _record)


# ---- the move mix (INTEGRATION.md "The move mix"): the stretch move, the differential-evolution move and the snooker move, one kind
#      per step chosen by weight.  The reference fits with DE at 0.8 and snooker at 0.2.  The numpy statement first, then the device. ----

MOVE_KINDS = ("stretch", "de", "snooker")  # VAG_MOVE_*
REFERENCE_MOVES = (("de", 0.8), ("snooker", 0.2))  # the reference's emcee configuration (config.py:160-161)
DE_SIGMA, SNOOKER_GAMMA = 1e-5, 1.7
_TWO_PI = 6.283185307179586  # vag::MOVE_TWO_PI


def move_weights(moves) -> np.ndarray:
    """(w_stretch, w_de, w_snooker) of ``moves``: "reference" (REFERENCE_MOVES) or a sequence of (name, weight) with names from
    MOVE_KINDS, each at most once.  The weights are non-negative and finite with a sum > 0; only their ratios matter."""
    if isinstance(moves, str):
        if moves != "reference":
            raise ValueError(f"unknown move mix {moves!r}: 'reference' or a sequence of (name, weight)")
        moves = REFERENCE_MOVES
    weights = np.zeros(3)
    seen = set()
    try:
        pairs = [(name, float(weight)) for name, weight in moves]
    except (TypeError, ValueError):
        raise ValueError("moves must be 'reference' or a sequence of (name, weight)") from None
    for name, weight in pairs:
        if name not in MOVE_KINDS:
            raise ValueError(f"unknown move {name!r}: one of {MOVE_KINDS}")
        if name in seen:
            raise ValueError(f"move {name!r} is listed twice")
        seen.add(name)
        weights[MOVE_KINDS.index(name)] = weight
    if not np.all(np.isfinite(weights)) or np.any(weights < 0.0):
        raise ValueError("move weights must be finite and >= 0")
    if not weights.sum() > 0.0:
        raise ValueError("move weights must not all be zero")
    return weights


def de_gamma0(ndim: int) -> float:
    """vag::de_gamma0: 2.38 / sqrt(2 ndim), the customary scale of the DE move."""
    return float(2.38 / np.sqrt(2.0 * ndim))


def _check_moves(weights, nwalkers, ndim, a=2.0, gamma0=None, sigma=DE_SIGMA, gamma_snooker=SNOOKER_GAMMA, thin=1):
    """The refusals of vag_move_spec on the Python side; returns gamma0 with None resolved."""
    _check_stretch(nwalkers, ndim, a, thin)
    if weights[1] > 0.0 and nwalkers // 2 < 2:
        raise ValueError("the DE move needs two walkers of the other half: at least 4 walkers")
    if weights[2] > 0.0 and nwalkers // 2 < 3:
        raise ValueError("the snooker move needs three walkers of the other half: at least 6 walkers")
    gamma0 = de_gamma0(ndim) if gamma0 is None else float(gamma0)
    if not (np.isfinite(gamma0) and gamma0 > 0.0):
        raise ValueError("gamma0 must be finite and > 0 (None: 2.38 / sqrt(2 ndim))")
    if not (np.isfinite(sigma) and np.isfinite(gamma_snooker)):
        raise ValueError("sigma and gamma_snooker must be finite")
    return gamma0


def move_kind(step, seed, weights) -> int:
    """vag::move_choice at absolute step `step`: 0 stretch, 1 DE, 2 snooker (the index into MOVE_KINDS).  One choice per step, shared
    by both halves: u of the first two words of counter (0, step lo, step hi, 3), times the sum of the weights, against the
    cumulative weights.  A kind of weight 0 is never chosen."""
    step, seed = int(step), int(seed)
    w0, w1, w2 = (float(w) for w in weights)
    x = philox4x32([0, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 3], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    c1 = w0 + w1
    t = float(_u53(x[0], x[1])) * (c1 + w2)
    if t < w0:
        return 0
    if t < c1:
        return 1
    return 2 if w2 > 0.0 else (1 if w1 > 0.0 else 0)


def _scaled_index(x, n):
    """vag::stretch_partner: (uint64(x) n) >> 32."""
    return ((x.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _move_pair(xa, xb, nh):
    """vag::move_pair: two distinct indices within a half of nh >= 2."""
    a = _scaled_index(xa, nh)
    return a, (a + 1 + _scaled_index(xb, nh - 1)) % nh


def _move_triple(xa, xb, xc, nh):
    """vag::move_triple: three distinct indices within a half of nh >= 3, the third stepped over the first two in ascending order."""
    a, b = _move_pair(xa, xb, nh)
    c = _scaled_index(xc, nh - 2)
    c = c + (c >= np.minimum(a, b))
    c = c + (c >= np.maximum(a, b))
    return a, b, c


def de_normal(u1, u2):
    """vag::de_quantise(vag::de_normal(u1, u2)) and its slack: the Box-Muller normal sqrt(-2 log(1 - u1)) cos(2 pi u2) rounded to a
    multiple of 2^-20, and the distance of n 2^20 from the nearest half-integer, in quanta.  The quantised value is the same on every
    machine whose log and cos round n 2^20 (below 2^24) to the same side of that half-integer: where the slack is far above their
    rounding (about 1e-9)."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    scaled = (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(_TWO_PI * u2)) * 2.0 ** 20
    return np.rint(scaled) * 2.0 ** -20, np.abs((scaled - np.floor(scaled)) - 0.5)


def de_proposals(pos, step, half, seed, gamma0=None, sigma=DE_SIGMA):
    """The DE proposals of half `half` at absolute step `step`: (prop[nw / 2, ndim], factor[nw / 2] = 0, partners[nw / 2, 2],
    slack[nw / 2]).  Walker w draws a != b of the other half (partners: their indices in the whole ensemble) from words 2 and 3 of
    stream 0 and a quantised normal n_q (de_normal: u1 from words 0, 1 of stream 0, u2 from words 0, 1 of stream 4);
    gamma = gamma0 fma(sigma, n_q, 1) and prop = fma(gamma, pos[a] - pos[b], pos[w]).  Bit for bit what vag_move_propose_dev computes
    on a DE step wherever the slack is far above the rounding of log and cos."""
    from .fitting import _fma
    pos = np.asarray(pos, dtype=np.float64)
    nw, ndim = pos.shape
    nh = nw // 2
    gamma0 = de_gamma0(ndim) if gamma0 is None else float(gamma0)
    x, v = _stretch_words(nw, step, half, seed, 0), _stretch_words(nw, step, half, seed, 4)
    a, b = _move_pair(x[:, 2], x[:, 3], nh)
    a, b = (1 - half) * nh + a, (1 - half) * nh + b
    n_q, slack = de_normal(_u53(x[:, 0], x[:, 1]), _u53(v[:, 0], v[:, 1]))
    gamma = gamma0 * _fma(sigma, n_q, 1.0)
    prop = _fma(gamma[:, None], pos[a] - pos[b], pos[half * nh:(half + 1) * nh])
    return prop, np.zeros(nh), np.stack([a, b], axis=1), slack


def snooker_proposals(pos, step, half, seed, gamma_snooker=SNOOKER_GAMMA):
    """The snooker proposals of half `half` at absolute step `step`: (prop[nw / 2, ndim], factor[nw / 2], partners[nw / 2, 3]).
    Walker w draws distinct z, z1, z2 of the other half (words 2, 3 of stream 0, word 2 of stream 4).  With delta = pos[w] - pos[z],
    r2 = delta . delta and proj = delta . (pos[z1] - pos[z2]), summed in dimension order with one fma per term,
    prop = fma(gamma_snooker (proj / r2), delta, pos[w]) -- the projection on the unit vector of ter Braak & Vrugt (2008), not
    emcee's delta / sqrt(|delta|) -- and factor = (ndim - 1) / 2 log(|prop - pos[z]|^2 / r2), the ln of the Hastings factor.  A walker
    with r2 = 0 or a factor that is not finite proposes its own position with factor -inf.  The proposals are bit for bit what
    vag_move_propose_dev computes on a snooker step; the factor differs by the rounding of the logarithm."""
    from .fitting import _fma
    pos = np.asarray(pos, dtype=np.float64)
    nw, ndim = pos.shape
    nh = nw // 2
    x, v = _stretch_words(nw, step, half, seed, 0), _stretch_words(nw, step, half, seed, 4)
    partners = (1 - half) * nh + np.stack(_move_triple(x[:, 2], x[:, 3], v[:, 2], nh), axis=1)
    mine = pos[half * nh:(half + 1) * nh]
    pz, p1, p2 = pos[partners[:, 0]], pos[partners[:, 1]], pos[partners[:, 2]]
    delta = mine - pz
    r2, proj = np.zeros(nh), np.zeros(nh)
    for d in range(ndim):
        r2 = _fma(delta[:, d], delta[:, d], r2)
        proj = _fma(delta[:, d], p1[:, d] - p2[:, d], proj)
    with np.errstate(all="ignore"):
        coef = gamma_snooker * (proj / r2)
        q = _fma(coef[:, None], delta, mine)
        e = q - pz
        q2 = np.zeros(nh)
        for d in range(ndim):
            q2 = _fma(e[:, d], e[:, d], q2)
        f = (0.5 * (ndim - 1.0)) * np.log(q2 / r2)
    ok = (r2 > 0.0) & np.isfinite(f)
    return np.where(ok[:, None], q, mine), np.where(ok, f, -np.inf), partners


def move_accepts(step, half, seed, factor, lp_new, lp_old):
    """The decisions of half `half` at step `step` for proposals of any kind: (take[nw / 2], margin[nw / 2]).  A proposal whose ln p
    is not finite, or whose factor is -inf, is rejected (margin -inf); any other is taken iff
    log(u_a) < factor + (lp_new - lp_old), u_a from stream 1 as in stretch_accepts, and margin is that right side minus the left."""
    factor, lp_new, lp_old = (np.asarray(v, dtype=np.float64) for v in (factor, lp_new, lp_old))
    y = _stretch_words(2 * factor.size, step, half, seed, 1)
    finite = np.isfinite(lp_new) & (factor > -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = (factor + (lp_new - lp_old)) - np.log(_u53(y[:, 0], y[:, 1]))  # (u_a = 0: log = -inf, taken)
    margin = np.where(finite, margin, -np.inf)
    return finite & (margin > 0), margin


def move_proposals(pos, step, half, seed, weights, a=2.0, gamma0=None, sigma=DE_SIGMA, gamma_snooker=SNOOKER_GAMMA):
    """The proposals of the kind chosen at `step` (move_kind): (prop, factor, kind, slack), slack None unless the kind is DE.  The
    stretch kind is stretch_proposals with factor = (ndim - 1) log z."""
    kind = move_kind(step, seed, weights)
    if kind == 0:
        prop, z, _ = stretch_proposals(pos, step, half, seed, a)
        return prop, (np.shape(pos)[1] - 1.0) * np.log(z), kind, None
    if kind == 1:
        prop, factor, _, slack = de_proposals(pos, step, half, seed, gamma0, sigma)
        return prop, factor, kind, slack
    prop, factor, _ = snooker_proposals(pos, step, half, seed, gamma_snooker)
    return prop, factor, kind, None


def run_moves_philox(log_prob_batch: Callable[[np.ndarray], np.ndarray], pos0: np.ndarray, nsteps: int, moves=REFERENCE_MOVES,
                     seed: int = 0, a: float = 2.0, gamma0: Optional[float] = None, sigma: float = DE_SIGMA,
                     gamma_snooker: float = SNOOKER_GAMMA, thin: int = 1, step0: int = 0, margins: Optional[list] = None,
                     slacks: Optional[list] = None):
    """run_stretch_move_philox with the move mix ``moves`` (move_weights): the chain of vag_move_run_dev through any host callable.
    Per step one kind (move_kind), per half its proposals (move_proposals) in one call of log_prob_batch and the decisions
    (move_accepts).  With only the stretch move the chain is run_stretch_move_philox's.

    Returns (chain[rows, nw, ndim], log_prob[rows, nw], acceptance[nw]).  ``margins`` receives every half-step's margin array,
    ``slacks`` every DE half-step's slack array (de_normal)."""
    weights = move_weights(moves)
    pos = np.array(pos0, dtype=np.float64, copy=True)
    nw, ndim = pos.shape
    gamma0 = _check_moves(weights, nw, ndim, a, gamma0, sigma, gamma_snooker, thin)
    lp = np.asarray(log_prob_batch(pos), dtype=np.float64).copy()
    if not np.all(np.isfinite(lp)):
        raise ValueError("initial positions must have finite log-probability")
    rows = (step0 + nsteps) // thin - step0 // thin
    chain, logp = np.empty((rows, nw, ndim)), np.empty((rows, nw))
    accepted = np.zeros(nw, dtype=np.int64)
    nh, row = nw // 2, 0
    for step in range(step0, step0 + nsteps):
        for half in (0, 1):
            s = slice(half * nh, (half + 1) * nh)
            prop, factor, _, slack = move_proposals(pos, step, half, seed, weights, a, gamma0, sigma, gamma_snooker)
            lp_new = np.asarray(log_prob_batch(prop), dtype=np.float64)
            take, margin = move_accepts(step, half, seed, factor, lp_new, lp[s])
            if margins is not None:
                margins.append(margin)
            if slacks is not None and slack is not None:
                slacks.append(slack)
            pos[s][take] = prop[take]
            lp[s][take] = lp_new[take]
            accepted[s][take] += 1
        if (step + 1) % thin == 0:
            chain[row], logp[row] = pos, lp
            row += 1
    return chain, logp, accepted / max(nsteps, 1)


def _move_spec(weights, nwalkers, ndim, seed, a, gamma0, sigma, gamma_snooker, thin):
    from . import _lib
    return _lib.MoveSpec(int(seed) & (2 ** 64 - 1), float(a), float(gamma0), float(sigma), float(gamma_snooker),
                         (_lib.C.c_double * 3)(*weights), int(nwalkers), int(ndim), int(thin))


class EnsembleMoves(_DeviceMove):
    """StretchMove for the move mix (vag_move_propose_dev / vag_move_accept_dev): the two halves of a half-step on float64 torch
    tensors and torch's current stream, with the ln of the Hastings factor between them; they need no model::

        move = EnsembleMoves(nw, ndim, moves=REFERENCE_MOVES, seed=7)
        for step in range(nsteps):
            for half in (0, 1):
                prop, factor = move.propose(step, half, pos)          # [nw / 2, ndim], [nw / 2]
                move.accept(step, half, prop, factor, evaluate(prop), pos, lp, accepted)   # pos, lp, accepted change in place

    ``move.kind(step)`` is the index into MOVE_KINDS of the move of that step.  The chain is the one run_moves_philox makes from the
    same ln p."""

    def __init__(self, nwalkers: int, ndim: int, moves=REFERENCE_MOVES, seed: int = 0, a: float = 2.0, gamma0: Optional[float] = None,
                 sigma: float = DE_SIGMA, gamma_snooker: float = SNOOKER_GAMMA, device: int = 0):
        self.weights = move_weights(moves)
        gamma0 = _check_moves(self.weights, nwalkers, ndim, a, gamma0, sigma, gamma_snooker)
        self.nwalkers, self.ndim, self.seed = int(nwalkers), int(ndim), int(seed)
        from . import _lib
        super().__init__(_lib.move_entry, _move_spec(self.weights, nwalkers, ndim, seed, a, gamma0, sigma, gamma_snooker, 1), device,
                         propose="vag_move_propose_dev", accept="vag_move_accept_dev")

    def kind(self, step: int) -> int:
        return move_kind(step, self.seed, self.weights)

    def propose(self, step: int, half: int, pos):
        import torch
        nh = self.nwalkers // 2
        self._checked(pos, (self.nwalkers, self.ndim), torch.float64, "pos")
        prop = torch.empty((nh, self.ndim), dtype=torch.float64, device=self._dev)
        factor = torch.empty((nh,), dtype=torch.float64, device=self._dev)
        self._call(self._propose, step, half, pos, prop, factor)
        return prop, factor

    def accept(self, step: int, half: int, prop, factor, lp_new, pos, lp, accepted):
        import torch
        nh = self.nwalkers // 2
        self._checked(prop, (nh, self.ndim), torch.float64, "prop")
        self._checked(factor, (nh,), torch.float64, "factor")
        self._checked(lp_new, (nh,), torch.float64, "lp_new")
        self._checked(pos, (self.nwalkers, self.ndim), torch.float64, "pos")
        self._checked(lp, (self.nwalkers,), torch.float64, "lp")
        self._checked(accepted, (self.nwalkers,), torch.int64, "accepted")
        self._call(self._accept, step, half, prop, factor, lp_new, pos, lp, accepted)


def run_moves_device(fitter: Fitter, param_defs: Sequence[ParamDef], pos0: np.ndarray, nsteps: int, moves=REFERENCE_MOVES,
                     seed: int = 0, a: float = 2.0, gamma0: Optional[float] = None, sigma: float = DE_SIGMA,
                     gamma_snooker: float = SNOOKER_GAMMA, thin: int = 1, priors=None, chunk: int = 64,
                     progress: Optional[Callable] = None, converge: Optional["Convergence"] = None, nburn: int = 0, _record: bool = False):
    """run_stretch_move_device with the move mix ``moves`` (move_weights; the default is the reference's DE 0.8 / snooker 0.2): every
    `chunk` steps are ONE call of vag_move_run_dev, which chooses each step's kind on the host and launches its kernels around the
    likelihood call.  Returns, chunking, thinning, ``progress``, ``converge`` and ``nburn`` as there; the chain is run_moves_philox's
    from the same ln p."""
    weights = move_weights(moves)

    def make_move(nw, ndim):
        g0 = _check_moves(weights, nw, ndim, a, gamma0, sigma, gamma_snooker, thin)
        return _move_spec(weights, nw, ndim, seed, a, g0, sigma, gamma_snooker, thin)
    return _run_halves_device(fitter, param_defs, pos0, nsteps, thin, priors, chunk, progress, "run_moves_device", "vag_move_run_dev",
                              make_move, converge, nburn, _record)


# ---- parallel tempering around that move (INTEGRATION.md "Parallel tempering"): a ladder of T inverse temperatures, temperature t
#      sampling beta_t ln L + ln prior with an ensemble of its own, exchanges between neighbours, the evidence by thermodynamic
#      integration.  The numpy statement first, then the device. ----

TEMPER_MAX = 64  # VAG_TEMPER_MAX


def geometric_betas(ntemps: int, beta_min: float = 1e-3, prior_rung: bool = False) -> np.ndarray:
    """The ladder beta_t = beta_min ** (t / (ntemps - 1)), t = 0 .. ntemps - 1: from 1 down to beta_min in equal ratios.  With
    ``prior_rung`` the last rung is 0 (the prior) and the others are spread over ntemps - 1: beta_min ** (t / (ntemps - 2))."""
    ntemps = int(ntemps)
    if not 1 <= ntemps <= TEMPER_MAX:
        raise ValueError(f"ntemps must be 1..{TEMPER_MAX}")
    if not (np.isfinite(beta_min) and 0.0 < beta_min < 1.0):
        raise ValueError("beta_min must lie in (0, 1)")
    n = ntemps - 1 if prior_rung else ntemps
    if prior_rung and ntemps < 2:
        raise ValueError("a ladder with a prior rung has at least two temperatures")
    betas = np.ones(n) if n == 1 else float(beta_min) ** (np.arange(n) / (n - 1.0))
    betas[0] = 1.0
    return np.append(betas, 0.0) if prior_rung else betas


def _check_betas(betas) -> np.ndarray:
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    if betas.ndim != 1 or not 1 <= betas.size <= TEMPER_MAX:
        raise ValueError(f"betas must hold 1..{TEMPER_MAX} inverse temperatures")
    if betas[0] != 1.0:
        raise ValueError("betas must start at 1")
    if not np.all(np.isfinite(betas)) or np.any(np.diff(betas) >= 0.0) or betas[-1] < 0.0:
        raise ValueError("betas must be finite, strictly descending and >= 0")
    return betas


def _tempered_words(ntemps, nwalkers, walkers, step, seed, stream):
    """The four Philox words of the replicas r = t nwalkers + w, w in `walkers`, of every temperature: uint32[T, len(walkers), 4]."""
    step, seed = int(step), int(seed)
    r = (np.arange(ntemps, dtype=np.uint64)[:, None] * np.uint64(nwalkers) + np.asarray(walkers, dtype=np.uint64)[None, :])
    counter = np.empty(r.shape + (4,), dtype=np.uint64)
    counter[..., 0] = r
    counter[..., 1], counter[..., 2], counter[..., 3] = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, stream
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))


def tempered_log_ratio(beta, lnl_new, lnl_old, lnprior_new, lnprior_old):
    """vag::tempered_log_ratio in numpy: fma(beta, lnl_new - lnl_old, lnprior_new - lnprior_old)."""
    from .fitting import _fma
    lnl_new, lnl_old, lnprior_new, lnprior_old = (np.asarray(v, dtype=np.float64) for v in (lnl_new, lnl_old, lnprior_new, lnprior_old))
    return _fma(beta, lnl_new - lnl_old, lnprior_new - lnprior_old)


def swap_log_ratio(beta_lo, beta_hi, lnl_lo, lnl_hi):
    """vag::swap_log_ratio in numpy: (beta_lo - beta_hi) (lnl_hi - lnl_lo)."""
    return (np.asarray(beta_lo, dtype=np.float64) - beta_hi) * (np.asarray(lnl_hi, dtype=np.float64) - lnl_lo)


def tempered_proposals(pos, step, half, seed, a=2.0):
    """The proposals of half `half` of every temperature at absolute step `step`, from pos[T, nw, ndim]:
    (prop[T, nw / 2, ndim], z[T, nw / 2], partner[T, nw / 2]), partner the index within the temperature's ensemble.  Bit for bit
    what vag_tempered_propose_dev computes."""
    from .fitting import _fma
    pos = np.asarray(pos, dtype=np.float64)
    ntemps, nw, _ = pos.shape
    nh = nw // 2
    x = _tempered_words(ntemps, nw, half * nh + np.arange(nh), step, seed, 0)
    z = stretch_z(a, _u53(x[..., 0], x[..., 1]))
    partner = (1 - half) * nh + ((x[..., 2].astype(np.uint64) * np.uint64(nh)) >> np.uint64(32)).astype(np.int64)
    other = np.take_along_axis(pos, partner[..., None], axis=1)
    return _fma(z[..., None], pos[:, half * nh:(half + 1) * nh] - other, other), z, partner


def tempered_accepts(step, half, seed, z, betas, lnl_new, lnprior_new, lnl_old, lnprior_old, ndim):
    """The decisions of half `half` of every temperature at step `step`: (take[T, nw / 2], margin[T, nw / 2]).  A proposal whose
    ln L or ln prior is not finite is rejected at every temperature (margin -inf); any other is taken iff
    log(u_a) < (ndim - 1) log z + fma(beta_t, lnl_new - lnl_old, lnprior_new - lnprior_old), and margin is that right side minus the
    left, as in stretch_accepts."""
    z, lnl_new, lnprior_new, lnl_old, lnprior_old = (np.asarray(v, dtype=np.float64) for v in (z, lnl_new, lnprior_new, lnl_old, lnprior_old))
    ntemps, nh = z.shape
    y = _tempered_words(ntemps, 2 * nh, half * nh + np.arange(nh), step, seed, 1)
    finite = np.isfinite(lnl_new) & np.isfinite(lnprior_new)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = tempered_log_ratio(np.asarray(betas, dtype=np.float64)[:, None], np.where(finite, lnl_new, 0.0), lnl_old,
                                   np.where(finite, lnprior_new, 0.0), lnprior_old)
        margin = ((ndim - 1.0) * np.log(z) + ratio) - np.log(_u53(y[..., 0], y[..., 1]))  # (u_a = 0: log = -inf, taken)
    margin = np.where(finite, margin, -np.inf)
    return finite & (margin > 0), margin


def tempered_swaps(step, seed, betas, lnl):
    """The exchanges of step `step` from lnl[T, nw]: (lower[npairs], take[npairs, nw], margin[npairs, nw]).  lower holds the t of
    the attempted pairs (t, t + 1), those with t + step even; walker w of t pairs with walker w of t + 1 and they exchange iff
    log(u_s) < (beta_t - beta_t+1) (lnl[t + 1, w] - lnl[t, w]), u_s from stream 2 at r = t nw + w; margin is the right side minus
    the left."""
    betas, lnl = np.asarray(betas, dtype=np.float64), np.asarray(lnl, dtype=np.float64)
    ntemps, nw = lnl.shape
    lower = np.arange(int(step) & 1, ntemps - 1, 2)
    y = _tempered_words(ntemps, nw, np.arange(nw), step, seed, 2)[lower]
    with np.errstate(divide="ignore"):
        margin = swap_log_ratio(betas[lower, None], betas[lower + 1, None], lnl[lower], lnl[lower + 1]) - np.log(_u53(y[..., 0], y[..., 1]))
    return lower, margin > 0, margin


def swap_attempts(ntemps, step0, nsteps):
    """How often each pair (t, t + 1) is attempted in steps step0 .. step0 + nsteps - 1: the steps s with t + s even."""
    t = np.arange(max(ntemps - 1, 0))
    first = step0 + ((t + step0) & 1)  # the first such step
    return np.maximum(0, (step0 + nsteps - first + 1) // 2)


def run_tempered_philox(log_like_batch: Callable[[np.ndarray], np.ndarray], log_prior_batch: Callable[[np.ndarray], np.ndarray],
                        pos0: np.ndarray, betas, nsteps: int, seed: int = 0, a: float = 2.0, thin: int = 1, step0: int = 0,
                        margins: Optional[list] = None):
    """Parallel tempering through any two host callables (ln L and ln prior of rows [n, ndim]): the chain of the device's tempered
    sampler.  pos0[T, nw, ndim]; a step is half 0 and half 1 of every temperature (the stretch move with fixed halves on
    beta_t ln L + ln prior, the T nw / 2 proposals in one call of each callable), then the exchanges of tempered_swaps.  Runs steps
    step0 .. step0 + nsteps - 1 and stores step s, the state after its exchanges, when (s + 1) % thin == 0.

    Returns (chain[rows, T, nw, ndim], lnl[rows, T, nw], lnprior[rows, T, nw], acceptance[T, nw], swap_fraction[T - 1]):
    swap_fraction is accepted over attempted exchanges of the pair (t, t + 1).  ``margins``: a list that receives every half-step's
    and every exchange phase's margin array."""
    pos = np.array(pos0, dtype=np.float64, copy=True)
    if pos.ndim != 3:
        raise ValueError("pos0 must be [ntemps, nwalkers, ndim]")
    betas = _check_betas(betas)
    ntemps, nw, ndim = pos.shape
    if ntemps != betas.size:
        raise ValueError("pos0 must be [ntemps, nwalkers, ndim] with one ensemble per entry of betas")
    _check_stretch(nw, ndim, a, thin)
    lnl = np.asarray(log_like_batch(pos.reshape(-1, ndim)), dtype=np.float64).reshape(ntemps, nw).copy()
    lnprior = np.asarray(log_prior_batch(pos.reshape(-1, ndim)), dtype=np.float64).reshape(ntemps, nw).copy()
    if not (np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnprior))):
        raise ValueError("initial positions must have finite ln L and ln prior")
    rows = (step0 + nsteps) // thin - step0 // thin
    chain, lnl_chain, lnprior_chain = np.empty((rows, ntemps, nw, ndim)), np.empty((rows, ntemps, nw)), np.empty((rows, ntemps, nw))
    accepted = np.zeros((ntemps, nw), dtype=np.int64)
    swapped = np.zeros((max(ntemps - 1, 1), nw), dtype=np.int64)
    nh, row = nw // 2, 0
    for step in range(step0, step0 + nsteps):
        for half in (0, 1):
            s = slice(half * nh, (half + 1) * nh)
            prop, z, _ = tempered_proposals(pos, step, half, seed, a)
            flat = prop.reshape(-1, ndim)
            lnl_new = np.asarray(log_like_batch(flat), dtype=np.float64).reshape(ntemps, nh)
            lnprior_new = np.asarray(log_prior_batch(flat), dtype=np.float64).reshape(ntemps, nh)
            take, margin = tempered_accepts(step, half, seed, z, betas, lnl_new, lnprior_new, lnl[:, s], lnprior[:, s], ndim)
            if margins is not None:
                margins.append(margin)
            pos[:, s][take] = prop[take]
            lnl[:, s][take] = lnl_new[take]
            lnprior[:, s][take] = lnprior_new[take]
            accepted[:, s][take] += 1
        if ntemps > 1:
            lower, take, margin = tempered_swaps(step, seed, betas, lnl)
            if margins is not None:
                margins.append(margin)
            for k, t in enumerate(lower):
                w = take[k]
                for arr in (pos, lnl, lnprior):
                    arr[t, w], arr[t + 1, w] = arr[t + 1, w].copy(), arr[t, w].copy()
                swapped[t, w] += 1
        if (step + 1) % thin == 0:
            chain[row], lnl_chain[row], lnprior_chain[row] = pos, lnl, lnprior
            row += 1
    attempts = swap_attempts(ntemps, step0, nsteps)
    swap_fraction = swapped[:ntemps - 1].sum(axis=1) / np.maximum(attempts * nw, 1)
    return chain, lnl_chain, lnprior_chain, accepted / max(nsteps, 1), swap_fraction


def thermodynamic_evidence(betas, mean_lnl):
    """ln Z = integral over beta from 0 to 1 of <ln L>_beta by thermodynamic integration: the trapezoid rule over the ladder on
    mean_lnl[T], the mean of ln L at each rung (after burn-in).  Returns (ln_z, error_estimate), the estimate being the difference
    to the same rule on every second rung, as ptemcee does.

    The integral runs from 0: the ladder must reach beta = 0 (geometric_betas(..., prior_rung=True)) or close to it for the number
    to mean anything -- the part below the last rung is simply missing.  The estimate says nothing about that, and the rule's
    discretisation error (<ln L>_beta is steep towards small beta) is the caller's to control through the ladder."""
    betas, mean_lnl = np.asarray(betas, dtype=np.float64), np.asarray(mean_lnl, dtype=np.float64)
    if betas.ndim != 1 or betas.shape != mean_lnl.shape:
        raise ValueError("betas and mean_lnl must be one value per rung")

    def trapezoid(b, m):  # (descending beta: the differences are negative)
        return float(-np.sum(np.diff(b) * 0.5 * (m[1:] + m[:-1])))
    ln_z = trapezoid(betas, mean_lnl)
    coarse = np.arange(0, betas.size, 2)
    if coarse[-1] != betas.size - 1:
        coarse = np.append(coarse, betas.size - 1)  # (both rules cover the same range)
    return ln_z, abs(ln_z - trapezoid(betas[coarse], mean_lnl[coarse]))


class TemperedMove(_DeviceMove):
    """The building blocks of a tempered step on the device (vag_tempered_propose_dev / _accept_dev / _swap_dev), on float64 torch
    tensors and torch's current stream, like StretchMove; they need no model::

        move = TemperedMove(betas, nw, ndim, seed=7)
        for step in range(nsteps):
            for half in (0, 1):
                prop = move.propose(step, half, pos)                      # [T, nw / 2, ndim] from pos[T, nw, ndim]
                lnl_new, lnprior_new = evaluate(prop.reshape(-1, ndim))   # any float64[T * nw / 2] pair on the device
                move.accept(step, half, prop, lnl_new.reshape(T, -1), lnprior_new.reshape(T, -1), pos, lnl, lnprior, accepted)
            move.swap(step, pos, lnl, lnprior, swapped)                   # swapped: int64[max(T - 1, 1), nw]

    The chain is the one sampling.run_tempered_philox makes from the same ln L and ln prior."""

    def __init__(self, betas, nwalkers: int, ndim: int, seed: int = 0, a: float = 2.0, device: int = 0):
        self.betas = _check_betas(betas)
        _check_stretch(nwalkers, ndim, a)
        import ctypes as C
        from . import _lib
        self.ntemps, self.nwalkers, self.ndim = int(self.betas.size), int(nwalkers), int(ndim)
        spec = _lib.TemperedSpec(int(seed) & (2 ** 64 - 1), float(a), self.ntemps, self.nwalkers, self.ndim, 1,
                                 self.betas.ctypes.data_as(C.POINTER(C.c_double)))
        super().__init__(_lib.tempered_entry, spec, device, propose="vag_tempered_propose_dev", accept="vag_tempered_accept_dev",
                         swap="vag_tempered_swap_dev")

    def propose(self, step: int, half: int, pos):
        import torch
        self._checked(pos, (self.ntemps, self.nwalkers, self.ndim), torch.float64, "pos")
        prop = torch.empty((self.ntemps, self.nwalkers // 2, self.ndim), dtype=torch.float64, device=self._dev)
        self._call(self._propose, step, half, pos, prop)
        return prop

    def accept(self, step: int, half: int, prop, lnl_new, lnprior_new, pos, lnl, lnprior, accepted):
        import torch
        T, nw, nh = self.ntemps, self.nwalkers, self.nwalkers // 2
        self._checked(prop, (T, nh, self.ndim), torch.float64, "prop")
        self._checked(lnl_new, (T, nh), torch.float64, "lnl_new")
        self._checked(lnprior_new, (T, nh), torch.float64, "lnprior_new")
        self._checked(pos, (T, nw, self.ndim), torch.float64, "pos")
        self._checked(lnl, (T, nw), torch.float64, "lnl")
        self._checked(lnprior, (T, nw), torch.float64, "lnprior")
        self._checked(accepted, (T, nw), torch.int64, "accepted")
        self._call(self._accept, step, half, prop, lnl_new, lnprior_new, pos, lnl, lnprior, accepted)

    def swap(self, step: int, pos, lnl, lnprior, swapped):
        import torch
        T, nw = self.ntemps, self.nwalkers
        self._checked(pos, (T, nw, self.ndim), torch.float64, "pos")
        self._checked(lnl, (T, nw), torch.float64, "lnl")
        self._checked(lnprior, (T, nw), torch.float64, "lnprior")
        self._checked(swapped, (max(T - 1, 1), nw), torch.int64, "swapped")
        self._call(self._swap, step, pos, lnl, lnprior, swapped)


def loglike_split_device(fitter: Fitter, spec, theta, lnl, lnprior):
    """vag_loglike_split_dev on float64 device tensors and torch's current stream: ln L and ln prior of theta[nb, ndim] into
    lnl[nb] and lnprior[nb], for a spec made by Fitter.build_spec (use_priors=True for a prior other than 0)."""
    import ctypes as C
    import torch
    from . import _lib
    from .fitting import loglike_request, on_current_stream
    from .model import get_context
    lib = _lib.load()
    split = _lib.tempered_entry(lib, "vag_loglike_split_dev")
    h, lock = get_context(fitter.device)
    dev = torch.device("cuda", fitter.device)
    nb = int(theta.shape[0])
    for t, shape, what in ((theta, (nb, spec.ndim), "theta"), (lnl, (nb,), "lnl"), (lnprior, (nb,), "lnprior")):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float64 tensor {shape} on {dev}")
    request = loglike_request(spec)
    on_current_stream(lib, h, lock, dev, lambda: _lib.check(split(h, C.byref(request), theta.data_ptr(), nb, spec.ndim, lnl.data_ptr(),
                                                                   lnprior.data_ptr())))


def run_tempered_device(fitter: Fitter, param_defs: Sequence[ParamDef], pos0: np.ndarray, betas, nsteps: int, seed: int = 0,
                        a: float = 2.0, thin: int = 1, priors=None, chunk: int = 64, progress: Optional[Callable] = None,
                        converge: Optional["Convergence"] = None, nburn: int = 0, _record: bool = False):
    """run_tempered_philox with everything on the device: the spec is built once, and every `chunk` steps are ONE call
    (vag_tempered_run_dev) that scans and uploads the spec blocks once and then only launches.  Per half-step the T nw / 2 proposals
    of all temperatures go through one likelihood call; positions, ln L, ln prior, the chain and the counts stay in HBM.  ln L is the
    fitter's, ln prior the sum of the priors with the bounds mask (Fitter.log_like_and_prior_batch); only priors that run on the
    device are accepted.

    Returns (chain[nsteps // thin, T, nw, ndim], lnl[.., T, nw], lnprior[.., T, nw], acceptance[T, nw], swap_fraction[T - 1]) as
    numpy arrays.  The chunk size does not change a bit of them.  ``progress(step, pos, lnl, lnprior)`` is called once per chunk
    with the last step of the chunk; the context's lock is free between chunks.

    ``converge`` and ``nburn`` as in run_stretch_move_device, with the autocorrelation times of the cold rung (beta = 1), read in
    place through its row stride: ``nsteps`` is then a maximum, the five values are those of a plain run of the steps run, and a
    sixth follows, the ConvergedAutocorr record."""
    import ctypes as C
    from . import _lib
    pos0 = np.ascontiguousarray(pos0, dtype=np.float64)
    if pos0.ndim != 3:
        raise ValueError("pos0 must be [ntemps, nwalkers, ndim]")
    betas = _check_betas(betas)
    ntemps, nw, ndim = pos0.shape
    if ntemps != betas.size:
        raise ValueError("pos0 must be [ntemps, nwalkers, ndim] with one ensemble per entry of betas")
    _check_stretch(nw, ndim, a, thin)
    tempered = _lib.TemperedSpec(int(seed) & (2 ** 64 - 1), float(a), ntemps, nw, ndim, int(thin),
                                 betas.ctypes.data_as(C.POINTER(C.c_double)))

    def begin(lib, h, lock, dev, spec, rows):
        import torch
        pos = torch.from_numpy(pos0).to(dev)
        lnl = torch.empty((ntemps, nw), dtype=torch.float64, device=dev)
        lnprior = torch.empty((ntemps, nw), dtype=torch.float64, device=dev)
        accepted = torch.zeros((ntemps, nw), dtype=torch.int64, device=dev)
        swapped = torch.zeros((max(ntemps - 1, 1), nw), dtype=torch.int64, device=dev)
        chains = [torch.empty((rows, ntemps, nw) + tail, dtype=torch.float64, device=dev) for tail in ((ndim,), (), ())]
        loglike_split_device(fitter, spec, pos.view(-1, ndim), lnl.view(-1), lnprior.view(-1))
        if not bool((torch.isfinite(lnl) & torch.isfinite(lnprior)).all()):
            raise ValueError("initial positions must have finite ln L and ln prior")
        return [pos, lnl, lnprior], [accepted, swapped], chains
    chains, (accepted, swapped), ran, rec, _ = _run_chunks(
        fitter, param_defs, priors, "run_tempered_device", "pos0 must be [ntemps, nwalkers, ndim]", ndim, ntemps * nw // 2, nsteps, thin,
        chunk, progress, converge, nburn, _record, lambda kept: kept[:, 0],
        lambda lib: _lib.tempered_entry(lib, "vag_tempered_run_dev"), tempered, begin)
    swap_fraction = swapped[:ntemps - 1].sum(axis=1) / np.maximum(swap_attempts(ntemps, 0, ran) * nw, 1)
    out = (*chains, accepted / max(ran, 1), swap_fraction)
    return out if rec is None else out + (rec,)


# ---- nested sampling (INTEGRATION.md "Nested sampling"): N live points; an iteration retires the K = N / 2 of lowest ln L and replaces
#      each by a clone of a survivor that walks `walk` constrained DE steps against the survivors; the evidence from the stored ln L.
#      The numpy statement first, then the device. ----

NESTED_MAX_LIVE = 16384  # VAG_NESTED_MAX_LIVE
_NESTED_STREAM_CLONE = 5  # vag::NESTED_STREAM_CLONE

NestedRun = namedtuple("NestedRun", "dead_theta dead_lnl dead_lnprior live lnl lnprior accepted niter ncall")
NestedRun.__doc__ = """What run_nested_philox and run_nested_device return: the dead record dead_theta[niter, K, ndim], dead_lnl[niter, K],
dead_lnprior[niter, K] (row = iteration, in rank order: flattened it is non-decreasing in ln L), the final live points live[N, ndim]
with lnl[N] and lnprior[N], accepted[niter] (the taken proposals of each iteration, of K walk), the iterations run and the likelihood
evaluations N + niter K walk."""

NestedEvidence = namedtuple("NestedEvidence", "ln_z ln_z_err information log_weights")
NestedEvidence.__doc__ = """What nested_evidence returns: ln Z, its error sqrt(H / N), the information H, and the normalised log weights
of the flattened dead points followed by the final live points (their exponentials sum to 1)."""


def nested_default_walk(ndim: int) -> int:
    """The default walk length: max(20, 5 ndim) -- a short walk is visibly biased, and the bias grows with the dimension."""
    return max(20, 5 * int(ndim))


def _check_nested(n_live, ndim, walk, gamma0=None, sigma=DE_SIGMA):
    """The refusals of vag_nested_spec on the Python side; returns gamma0 with None resolved."""
    if n_live % 2 or not 4 <= n_live <= NESTED_MAX_LIVE:
        raise ValueError(f"need an even number of live points, 4..{NESTED_MAX_LIVE}")
    if not 1 <= ndim <= 16:
        raise ValueError("nested sampling takes 1..16 dimensions")
    if int(walk) != walk or walk < 1:
        raise ValueError("walk must be a whole number >= 1")
    gamma0 = de_gamma0(ndim) if gamma0 is None else float(gamma0)
    if not (np.isfinite(gamma0) and gamma0 > 0.0):
        raise ValueError("gamma0 must be finite and > 0 (None: 2.38 / sqrt(2 ndim))")
    if not np.isfinite(sigma):
        raise ValueError("sigma must be finite")
    return gamma0


def nested_tick(it: int, walk: int, m: int) -> int:
    """vag::nested_tick: the tick of draw m of iteration `it`, it (walk + 1) + m; m = 0 the clone draw, m = 1 .. walk the walk steps."""
    return int(it) * (int(walk) + 1) + int(m)


def _nested_words(k, tick, seed, stream):
    """The four Philox words of the ranks r = 0 .. k - 1 at `tick`: counter (r, tick lo, tick hi, stream)."""
    return _stretch_words(2 * k, tick, 0, seed, stream)


def nested_order(lnl):
    """(order[N], lstar): order[r] the live slot of rank r, slot i before slot j iff (lnl[i], i) < (lnl[j], j), so ties go to the lower
    slot; the dead are ranks 0 .. K - 1, the survivors ranks K .. N - 1, and lstar = lnl[order[K - 1]].  What vag_nested_rank_dev writes."""
    lnl = np.asarray(lnl, dtype=np.float64)
    order = np.lexsort((np.arange(lnl.size), lnl))
    return order, float(lnl[order[lnl.size // 2 - 1]])


def nested_clones(order, it, walk, seed):
    """The slot each dead rank r = 0 .. K - 1 is overwritten from at iteration `it`: survivor order[K + j0], j0 = floor(u K) with u the
    uniform of the first two words of stream 5 at tick (it, 0).  What vag_nested_retire_dev copies."""
    order = np.asarray(order)
    k = order.size // 2
    x = _nested_words(k, nested_tick(it, walk, 0), seed, _NESTED_STREAM_CLONE)
    j0 = np.minimum((_u53(x[:, 0], x[:, 1]) * float(k)).astype(np.int64), k - 1)
    return order[k + j0]


def nested_proposals(live, order, it, m, walk, seed, gamma0=None, sigma=DE_SIGMA):
    """The proposals of walk step m = 1 .. walk of iteration `it`, after the retirement: (prop[K, ndim], partners[K, 2], slack[K]).
    Clone r (slot order[r]) draws survivors s1 != s2 = order[K + a], order[K + b] with (a, b) the pair of words 2 and 3 of stream 0
    over the K survivors (partners: their slots) and the quantised normal of de_normal (u1 from words 0, 1 of stream 0, u2 from words
    0, 1 of stream 4); gamma = gamma0 fma(sigma, n_q, 1) and prop = fma(gamma, live[s1] - live[s2], live[order[r]]).  Bit for bit what
    vag_nested_propose_dev computes wherever the slack is far above the rounding of log and cos."""
    from .fitting import _fma
    live, order = np.asarray(live, dtype=np.float64), np.asarray(order)
    n, ndim = live.shape
    k = n // 2
    gamma0 = de_gamma0(ndim) if gamma0 is None else float(gamma0)
    tick = nested_tick(it, walk, m)
    x, v = _nested_words(k, tick, seed, 0), _nested_words(k, tick, seed, 4)
    a, b = _move_pair(x[:, 2], x[:, 3], k)
    s1, s2 = order[k + a], order[k + b]
    n_q, slack = de_normal(_u53(x[:, 0], x[:, 1]), _u53(v[:, 0], v[:, 1]))
    gamma = gamma0 * _fma(sigma, n_q, 1.0)
    return _fma(gamma[:, None], live[s1] - live[s2], live[order[:k]]), np.stack([s1, s2], axis=1), slack


def nested_margin(lnl_new, lnprior_new, lnprior_old, lstar, log_u):
    """vag::nested_margin in numpy: -inf where ln L' or ln prior' is not finite or ln L' is not strictly above lstar, whatever the
    draw; otherwise (lnprior_new - lnprior_old) - log_u.  A proposal is taken iff its margin is > 0."""
    lnl_new, lnprior_new, lnprior_old, log_u = (np.asarray(v, dtype=np.float64) for v in (lnl_new, lnprior_new, lnprior_old, log_u))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lnl_new) & np.isfinite(lnprior_new) & (lnl_new > lstar)
        return np.where(ok, (np.where(ok, lnprior_new, 0.0) - lnprior_old) - log_u, -np.inf)


def nested_accepts(it, m, walk, seed, lnl_new, lnprior_new, lnprior_old, lstar):
    """The decisions of walk step m of iteration `it`: (take[K], margin[K]), u_a from the first two words of stream 1 at tick (it, m)
    (u_a = 0: log = -inf, taken).  lnprior_old[K]: the clones' ln prior in rank order.  What vag_nested_accept_dev decides."""
    lnl_new = np.asarray(lnl_new, dtype=np.float64)
    y = _nested_words(lnl_new.size, nested_tick(it, walk, m), seed, 1)
    with np.errstate(divide="ignore"):
        margin = nested_margin(lnl_new, lnprior_new, lnprior_old, lstar, np.log(_u53(y[:, 0], y[:, 1])))
    return margin > 0, margin


def nested_live_count(j, n_live):
    """vag::nested_live_count: the live count when dead point j (flattened index) leaves, N - (j mod K)."""
    return int(n_live) - np.asarray(j, dtype=np.int64) % (int(n_live) // 2)


def _nested_dead_terms(dead_lnl, n_live):
    """(ln w of the flattened dead points, ln X after the last of them): n_j = N - (j mod K), ln X_j = -sum_{i <= j} 1 / n_i with
    X_-1 = 1, ln w_j = lnl_j + ln X_{j-1} + ln(-expm1(-1 / n_j))."""
    lnl = np.asarray(dead_lnl, dtype=np.float64).ravel()
    shrink = 1.0 / nested_live_count(np.arange(lnl.size), n_live).astype(np.float64)
    ln_x = -np.cumsum(shrink)
    before = np.concatenate([[0.0], ln_x[:-1]])
    return lnl + before + np.log(-np.expm1(-shrink)), float(ln_x[-1]) if lnl.size else 0.0


def _logsumexp(x):
    top = np.max(x)
    return float(top + np.log(np.sum(np.exp(x - top))))


def nested_evidence(dead_lnl, live_lnl) -> NestedEvidence:
    """The evidence of a run from its stored ln L: dead_lnl[niter, K] (or flattened) and the N final live points' live_lnl[N].  Dead
    point j left n_j = N - (j mod K) live points: ln X_j = -sum_{i <= j} 1 / n_i, ln w_j = lnl_j + ln X_{j-1} + ln(1 - exp(-1 / n_j));
    each final live point gets lnl + ln X_last - ln N.  ln Z = logsumexp of all, H = sum p lnl - ln Z with p the normalised weights,
    and the error is sqrt(H / N) (Skilling 2006).  Returns NestedEvidence(ln_z, ln_z_err, information, log_weights)."""
    live_lnl = np.asarray(live_lnl, dtype=np.float64).ravel()
    n = live_lnl.size
    if n < 4 or n % 2:
        raise ValueError("live_lnl must hold the N final live points, N even and >= 4")
    dead = np.asarray(dead_lnl, dtype=np.float64).ravel()
    if dead.size % (n // 2):
        raise ValueError("dead_lnl must hold whole iterations of N / 2 points")
    ln_w_dead, ln_x_last = _nested_dead_terms(dead, n)
    ln_w = np.concatenate([ln_w_dead, live_lnl + ln_x_last - np.log(n)])
    ln_z = _logsumexp(ln_w)
    log_weights = ln_w - ln_z
    information = float(np.sum(np.exp(log_weights) * np.concatenate([dead, live_lnl])) - ln_z)
    return NestedEvidence(ln_z, math.sqrt(max(information, 0.0) / n), information, log_weights)


def nested_remaining(dead_lnl, live_lnl) -> float:
    """The termination measure after the iterations of dead_lnl: logaddexp(ln Z_dead, max(live lnl) + ln X_last) - ln Z_dead, an upper
    bound on what the live points can still add to ln Z.  A run under ``dlogz`` stops at the first chunk end where it is < dlogz."""
    live_lnl = np.asarray(live_lnl, dtype=np.float64).ravel()
    ln_w_dead, ln_x_last = _nested_dead_terms(dead_lnl, live_lnl.size)
    if not ln_w_dead.size:
        return math.inf
    ln_z_dead = _logsumexp(ln_w_dead)
    return float(np.logaddexp(ln_z_dead, live_lnl.max() + ln_x_last) - ln_z_dead)


def nested_equal_samples(log_weights, seed: int = 0, n: Optional[int] = None) -> np.ndarray:
    """Indices of n equally weighted draws (default: as many as there are weights) from the normalised log weights, by systematic
    resampling: the positions (u + i) / n, one uniform u from numpy's generator seeded by `seed`, through the cumulative weights."""
    p = np.exp(np.asarray(log_weights, dtype=np.float64))
    n = p.size if n is None else int(n)
    cum = np.cumsum(p)
    positions = (np.random.default_rng(seed).random() + np.arange(n)) / n * cum[-1]
    return np.minimum(np.searchsorted(cum, positions, side="right"), p.size - 1)


def _nested_stop(dlogz, niter, chunk):
    if chunk < 1 or niter < 0:
        raise ValueError("chunk must be >= 1 and niter >= 0")
    if dlogz is not None and not (np.isfinite(dlogz) and dlogz > 0.0):
        raise ValueError("dlogz must be finite and > 0, or None")


def run_nested_philox(log_like_batch: Callable[[np.ndarray], np.ndarray], log_prior_batch: Callable[[np.ndarray], np.ndarray],
                      live0: np.ndarray, niter: int, walk: int, seed: int = 0, it0: int = 0, margins: Optional[list] = None,
                      gamma0: Optional[float] = None, sigma: float = DE_SIGMA, dlogz: Optional[float] = None, chunk: int = 4,
                      slacks: Optional[list] = None) -> NestedRun:
    """Nested sampling through any two host callables (ln L and ln prior of rows [n, ndim]): the run of the device's nested sampler.
    live0[N, ndim], N even; iterations it0 .. it0 + niter - 1.  An iteration ranks the live points (nested_order), stores the K = N / 2
    of lowest ln L as its row of the dead record, overwrites each by a copy of a survivor (nested_clones), and runs `walk` steps on the K
    clones at once: the proposals of nested_proposals in rank order in one call of each callable, the decisions of nested_accepts
    against L* of the iteration.  The survivors do not move during an iteration.  The draws are a function of (seed, it, m, rank), so
    a continuation (it0 = the iterations run, live0 = the live points they left) repeats a single run to the bit.

    With ``dlogz`` niter is a maximum: after every `chunk` iterations the run stops if nested_remaining(dead so far of this call, live)
    < dlogz.  Returns a NestedRun.  ``margins`` receives every walk step's margin array, ``slacks`` its slack array (de_normal)."""
    live = np.array(live0, dtype=np.float64, copy=True)
    if live.ndim != 2:
        raise ValueError("live0 must be [n_live, ndim]")
    n, ndim = live.shape
    gamma0 = _check_nested(n, ndim, walk, gamma0, sigma)
    _nested_stop(dlogz, niter, chunk)
    lnl = np.asarray(log_like_batch(live), dtype=np.float64).copy()
    lnprior = np.asarray(log_prior_batch(live), dtype=np.float64).copy()
    if not (np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnprior))):
        raise ValueError("live points must have finite ln L and ln prior")
    k = n // 2
    dead_theta, dead_lnl, dead_lnprior = np.empty((niter, k, ndim)), np.empty((niter, k)), np.empty((niter, k))
    accepted = np.zeros(niter, dtype=np.int64)
    ran = 0
    for row in range(niter):
        it = it0 + row
        order, lstar = nested_order(lnl)
        dead, source = order[:k], nested_clones(order, it, walk, seed)
        dead_theta[row], dead_lnl[row], dead_lnprior[row] = live[dead], lnl[dead], lnprior[dead]
        live[dead], lnl[dead], lnprior[dead] = live[source], lnl[source], lnprior[source]
        for m in range(1, walk + 1):
            prop, _, slack = nested_proposals(live, order, it, m, walk, seed, gamma0, sigma)
            lnl_new = np.asarray(log_like_batch(prop), dtype=np.float64)
            lnprior_new = np.asarray(log_prior_batch(prop), dtype=np.float64)
            take, margin = nested_accepts(it, m, walk, seed, lnl_new, lnprior_new, lnprior[dead], lstar)
            if margins is not None:
                margins.append(margin)
            if slacks is not None:
                slacks.append(slack)
            live[dead[take]], lnl[dead[take]], lnprior[dead[take]] = prop[take], lnl_new[take], lnprior_new[take]
            accepted[row] += int(take.sum())
        ran = row + 1
        if dlogz is not None and (ran % chunk == 0 or ran == niter) and nested_remaining(dead_lnl[:ran], lnl) < dlogz:
            break
    return NestedRun(dead_theta[:ran], dead_lnl[:ran], dead_lnprior[:ran], live, lnl, lnprior, accepted[:ran], ran, n + ran * k * walk)


def _norm_cdf(x):
    """The standard normal CDF, 0.5 erfc(-x / sqrt 2), elementwise."""
    return 0.5 * np.vectorize(math.erfc, otypes=[np.float64])(-np.asarray(x, dtype=np.float64) / math.sqrt(2.0))


def _norm_ppf(p):
    """The inverse of _norm_cdf for p in (0, 1): Acklam's rational approximation (relative error 1.2e-9) and one step of Halley's
    method on the erfc form, which leaves the rounding of erfc."""
    p = np.asarray(p, dtype=np.float64)
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01,
         2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00,
         2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    with np.errstate(all="ignore"):
        q = p - 0.5
        r = q * q
        mid = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
              (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0)
        t = np.sqrt(-2.0 * np.log(np.minimum(p, 1.0 - p)))
        tail = (((((c[0] * t + c[1]) * t + c[2]) * t + c[3]) * t + c[4]) * t + c[5]) / ((((d[0] * t + d[1]) * t + d[2]) * t + d[3]) * t + 1.0)
        x = np.where(np.abs(q) <= 0.47575, mid, np.where(q < 0, tail, -tail))
        e = _norm_cdf(x) - p
        u = e * math.sqrt(2.0 * math.pi) * np.exp(0.5 * x * x)
        x = x - u / (1.0 + 0.5 * x * u)
    return x


def _prior_ranges(lower, upper, prior_specs, who):
    """Per dimension (kind, a, b, lo, hi): the prior the device evaluates and the part [lo, hi] of the box where it is not zero."""
    from . import _lib
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    if lower.shape != upper.shape or lower.ndim != 1 or len(prior_specs) != lower.size:
        raise ValueError("lower, upper and prior_specs must hold one entry per dimension")
    host = [d for d, spec in enumerate(prior_specs) if spec[0] == _lib.PRIOR_NONE]
    if host:
        raise ValueError(f"{who}: only Uniform / Gaussian / LogUniform priors (or their tuple forms) run on the device; "
                         f"got host-only priors for dimensions {host}")
    out = []
    for d, (kind, a, b, *_) in enumerate(prior_specs):
        lo, hi = float(lower[d]), float(upper[d])
        if kind in (_lib.PRIOR_UNIFORM_RANGE, _lib.PRIOR_LOG_UNIFORM):
            lo, hi = max(lo, float(a)), min(hi, float(b))
        if kind == _lib.PRIOR_LOG_UNIFORM and not a > 0.0:
            raise ValueError(f"{who}: a LogUniform prior needs a minimum > 0 (dimension {d})")
        if kind == _lib.PRIOR_GAUSSIAN and not b > 0.0:
            raise ValueError(f"{who}: a Gaussian prior needs sigma > 0 (dimension {d})")
        if not lo < hi:
            raise ValueError(f"{who}: the prior of dimension {d} has no support inside the bounds")
        out.append((kind, float(a), float(b), lo, hi))
    return out


def sample_prior(lower, upper, prior_specs, n: int, rng: np.random.Generator) -> np.ndarray:
    """n draws [n, ndim] from the priors the device evaluates, within the bounds: prior_specs[d] = (kind, a, b, ...) as Fitter.build_spec
    leaves them in ``fitter._prior_specs``.  Uniform: uniform over [lower, upper]; Uniform with its own range: over the part of it
    inside the bounds; Gaussian(a, b): truncated to the bounds, by the inverse CDF; LogUniform(a, b): uniform in ln x over the part of
    [a, b] inside the bounds.  Host-only priors are refused."""
    from . import _lib
    ranges = _prior_ranges(lower, upper, prior_specs, "sample_prior")
    out = np.empty((int(n), len(ranges)))
    for d, (kind, a, b, lo, hi) in enumerate(ranges):
        u = rng.random(int(n))
        if kind == _lib.PRIOR_GAUSSIAN:
            p_lo, p_hi = _norm_cdf((lo - a) / b), _norm_cdf((hi - a) / b)
            if not p_hi > p_lo:
                raise ValueError(f"sample_prior: the Gaussian prior of dimension {d} has no mass inside the bounds in double precision")
            x = a + b * _norm_ppf(p_lo + (p_hi - p_lo) * u)
        elif kind == _lib.PRIOR_LOG_UNIFORM:
            x = lo * np.exp(u * math.log(hi / lo))
        else:
            x = lo + (hi - lo) * u
        out[:, d] = np.clip(x, lo, hi)
    return out


def prior_mass(lower, upper, prior_specs) -> float:
    """The mass of the prior density, as the device evaluates it, inside the bounds: the product over the dimensions of 1 (Uniform:
    the density is 1 / (upper - lower)), the covered fraction of its own range (Uniform(a, b)), Phi((upper - a) / b) - Phi((lower - a) / b)
    (Gaussian(a, b)), ln(hi / lo) / ln(b / a) over the covered part [lo, hi] of [a, b] (LogUniform).  An evidence formed with these
    priors is relative to this mass."""
    from . import _lib
    mass = 1.0
    for kind, a, b, lo, hi in _prior_ranges(lower, upper, prior_specs, "prior_mass"):
        if kind == _lib.PRIOR_UNIFORM_RANGE:
            mass *= (hi - lo) / (b - a)
        elif kind == _lib.PRIOR_GAUSSIAN:
            mass *= float(_norm_cdf((hi - a) / b) - _norm_cdf((lo - a) / b))
        elif kind == _lib.PRIOR_LOG_UNIFORM:
            mass *= math.log(hi / lo) / math.log(b / a)
    return mass


def _nested_spec(n_live, ndim, walk, seed, gamma0, sigma):
    from . import _lib
    return _lib.NestedSpec(int(seed) & (2 ** 64 - 1), int(n_live), int(ndim), int(walk), 0, float(gamma0), float(sigma))


class NestedMove(_DeviceMove):
    """The building blocks of a nested iteration on the device (vag_nested_rank_dev / _retire_dev / _propose_dev / _accept_dev), on
    float64 torch tensors and torch's current stream, like StretchMove; they need no model::

        move = NestedMove(n, ndim, walk, seed=7)
        for it in range(niter):
            order, lstar = move.rank(lnl)                                          # int32[n], float64[1]
            move.retire(it, order, live, lnl, lnprior, dead_theta[it], dead_lnl[it], dead_lnprior[it])   # rows [n / 2, ...]
            for m in range(1, walk + 1):
                prop = move.propose(it, m, order, live)                            # [n / 2, ndim], in rank order
                lnl_new, lnprior_new = evaluate(prop)                              # any float64[n / 2] pair on the device
                move.accept(it, m, order, lstar, prop, lnl_new, lnprior_new, live, lnl, lnprior, accepted[it])   # int64[n / 2]

    The run is the one sampling.run_nested_philox makes from the same ln L and ln prior."""

    def __init__(self, n_live: int, ndim: int, walk: int, seed: int = 0, gamma0: Optional[float] = None, sigma: float = DE_SIGMA,
                 device: int = 0):
        gamma0 = _check_nested(n_live, ndim, walk, gamma0, sigma)
        from . import _lib
        self.n_live, self.ndim, self.walk = int(n_live), int(ndim), int(walk)
        super().__init__(_lib.nested_entry, _nested_spec(n_live, ndim, walk, seed, gamma0, sigma), device, rank="vag_nested_rank_dev",
                         retire="vag_nested_retire_dev", propose="vag_nested_propose_dev", accept="vag_nested_accept_dev")

    def _live(self, order, live=None, lnl=None, lnprior=None):
        import torch
        n = self.n_live
        for t, shape, dtype, what in ((order, (n,), torch.int32, "order"), (live, (n, self.ndim), torch.float64, "live"),
                                      (lnl, (n,), torch.float64, "lnl"), (lnprior, (n,), torch.float64, "lnprior")):
            if t is not None:
                self._checked(t, shape, dtype, what)

    def rank(self, lnl):
        import torch
        self._live(None, lnl=lnl)
        order = torch.empty((self.n_live,), dtype=torch.int32, device=self._dev)
        lstar = torch.empty((1,), dtype=torch.float64, device=self._dev)
        self._call(self._rank, lnl, order, lstar)
        return order, lstar

    def retire(self, it: int, order, live, lnl, lnprior, dead_theta, dead_lnl, dead_lnprior):
        import torch
        k = self.n_live // 2
        self._live(order, live, lnl, lnprior)
        self._checked(dead_theta, (k, self.ndim), torch.float64, "dead_theta")
        self._checked(dead_lnl, (k,), torch.float64, "dead_lnl")
        self._checked(dead_lnprior, (k,), torch.float64, "dead_lnprior")
        self._call(self._retire, it, order, live, lnl, lnprior, dead_theta, dead_lnl, dead_lnprior)

    def propose(self, it: int, m: int, order, live):
        import torch
        self._live(order, live)
        prop = torch.empty((self.n_live // 2, self.ndim), dtype=torch.float64, device=self._dev)
        self._call(self._propose, it, m, order, live, prop)
        return prop

    def accept(self, it: int, m: int, order, lstar, prop, lnl_new, lnprior_new, live, lnl, lnprior, accepted):
        import torch
        k = self.n_live // 2
        self._live(order, live, lnl, lnprior)
        self._checked(lstar, (1,), torch.float64, "lstar")
        self._checked(prop, (k, self.ndim), torch.float64, "prop")
        self._checked(lnl_new, (k,), torch.float64, "lnl_new")
        self._checked(lnprior_new, (k,), torch.float64, "lnprior_new")
        self._checked(accepted, (k,), torch.int64, "accepted")
        self._call(self._accept, it, m, order, lstar, prop, lnl_new, lnprior_new, live, lnl, lnprior, accepted)


def run_nested_device(fitter: Fitter, param_defs: Sequence[ParamDef], live0: np.ndarray, niter: int, walk: Optional[int] = None,
                      seed: int = 0, dlogz: Optional[float] = None, priors=None, chunk: int = 4, progress: Optional[Callable] = None,
                      gamma0: Optional[float] = None, sigma: float = DE_SIGMA) -> NestedRun:
    """run_nested_philox with everything on the device: the spec is built once, and every `chunk` iterations are ONE call
    (vag_nested_run_dev) that scans and uploads the spec blocks once and then only launches.  Per walk step the N / 2 proposals go
    through one likelihood call; the live points, the dead record and the counts stay in HBM.  ln L is the fitter's, ln prior the sum
    of the priors with the bounds mask (Fitter.log_like_and_prior_batch); only priors that run on the device are accepted.  The default
    ``walk`` is max(20, 5 ndim).

    With ``dlogz`` set, niter is a maximum and the rule (nested_remaining < dlogz) is tested at chunk ends, where ln L of the chunk's
    dead points and of the live points come to the host.  The arrays of a run are those of a plain run of the same number of
    iterations, to the bit, whatever the chunk.  ``progress(it, live, lnl, lnprior)`` is called once per chunk with the last iteration
    of the chunk; the context's lock is free between chunks.  Returns a NestedRun as numpy arrays."""
    from . import _lib
    live0 = np.ascontiguousarray(live0, dtype=np.float64)
    if live0.ndim != 2:
        raise ValueError("live0 must be [n_live, ndim]")
    n, ndim = live0.shape
    walk = nested_default_walk(ndim) if walk is None else walk
    gamma0 = _check_nested(n, ndim, walk, gamma0, sigma)
    _nested_stop(dlogz, niter, chunk)
    if not np.all(np.isfinite(live0)):
        raise ValueError("live points must be finite")
    k = n // 2
    nested = _nested_spec(n, ndim, walk, seed, gamma0, sigma)

    def begin(lib, h, lock, dev, spec, rows):
        import torch
        live = torch.from_numpy(live0).to(dev)
        lnl = torch.empty((n,), dtype=torch.float64, device=dev)
        lnprior = torch.empty((n,), dtype=torch.float64, device=dev)
        loglike_split_device(fitter, spec, live, lnl, lnprior)
        if not bool((torch.isfinite(lnl) & torch.isfinite(lnprior)).all()):
            raise ValueError("live points must have finite ln L and ln prior")
        accepted = torch.zeros((rows, k), dtype=torch.int64, device=dev)
        dead = [torch.empty((rows, k) + tail, dtype=torch.float64, device=dev) for tail in ((ndim,), (), ())]
        return [live, lnl, lnprior], [], [accepted] + dead

    def stop(state, chains, ran):
        return dlogz is not None and nested_remaining(chains[2][:ran].cpu().numpy(), state[1].cpu().numpy()) < dlogz
    (accepted, dead_theta, dead_lnl, dead_lnprior), _, ran, _, (live, lnl, lnprior) = _run_chunks(
        fitter, param_defs, priors, "run_nested_device", "live0 must be [n_live, ndim]", ndim, k, niter, 1, chunk, progress, None, 0, False,
        lambda kept: kept, lambda lib: _lib.nested_entry(lib, "vag_nested_run_dev"), nested, begin, stop=stop)
    return NestedRun(dead_theta, dead_lnl, dead_lnprior, live, lnl, lnprior, accepted.sum(axis=1), ran, n + ran * k * walk)


# ---- chain autocorrelation (INTEGRATION.md "Chain autocorrelation"): the integrated autocorrelation time of every parameter, pooled over
#      the walkers, with Sokal's window -- the number that says when a chain is long enough.  The numpy statement first, then the device,
#      then the stopping rule of the three device run drivers. ----

ChainAutocorr = namedtuple("ChainAutocorr", "tau window reliable rho n_rows max_lag")
ChainAutocorr.__doc__ = """What chain_autocorr and chain_autocorr_device return: tau[D] in stored rows (NaN where the pooled variance is
zero or not finite; a lower bound where window is -1), window[D] (Sokal's M, -1 = none within max_lag), reliable[D]
(window >= 0 and n_rows >= tol tau), rho[max_lag + 1, D] (None where it was not asked for), the rows used and the lag range."""

ConvergedAutocorr = namedtuple("ConvergedAutocorr", ChainAutocorr._fields + ("converged", "steps", "history", "thin"))
ConvergedAutocorr.__doc__ = """The last element a device run driver returns under ``converge=``: the estimate at the end of the run,
``converged`` (the stopping rule was met), ``steps`` (the steps run), ``history`` ([checks, D]: tau in rows at every check, NaN rows
where fewer than two rows were kept) and ``thin``; tau * thin is tau in steps."""


class Convergence:
    """The stopping rule of the device run drivers (``converge=``): every ``check`` steps the autocorrelation times of the rows kept
    so far are estimated on the device, and the run stops at the first check where every parameter is reliable (a window was found and
    rows >= tol tau) and no tau moved by more than rtol tau since the check before.  c is Sokal's window constant."""

    def __init__(self, check: int = 100, tol: float = 50.0, rtol: float = 0.01, c: float = 5.0):
        if int(check) != check or check < 1:
            raise ValueError("Convergence: check must be a whole number of steps >= 1")
        for name, v in (("tol", tol), ("rtol", rtol), ("c", c)):
            if not np.isfinite(v) or not v > 0:
                raise ValueError(f"Convergence: {name} must be finite and > 0, got {v}")
        self.check, self.tol, self.rtol, self.c = int(check), float(tol), float(rtol), float(c)

    def __repr__(self):
        return f"Convergence(check={self.check}, tol={self.tol}, rtol={self.rtol}, c={self.c})"

    def met(self, tau, reliable, previous) -> bool:
        """The rule at one check: tau[D] and reliable[D] of this check, ``previous`` the tau of the check before (None at the first)."""
        if previous is None or not np.all(reliable):
            return False
        return bool(np.all(np.abs(tau - previous) <= self.rtol * tau))


def default_max_lag(n_rows: int, c: float = 5.0, tol: float = 50.0) -> int:
    """L = min(n - 1, ceil(c n / tol)): a window beyond it means tau > n / tol, which fails the tol tau rule whatever it is."""
    return int(min(n_rows - 1, math.ceil(c * n_rows / tol)))


def _chain_lags(n, c, tol, max_lag):
    if not np.isfinite(c) or not c > 0 or not np.isfinite(tol) or not tol > 0:
        raise ValueError("chain autocorrelation: c and tol must be finite and > 0")
    if n < 2:
        raise ValueError(f"chain autocorrelation: at least two rows are needed, got {n}")
    if max_lag is None:
        return default_max_lag(n, c, tol)
    if int(max_lag) != max_lag or not 1 <= max_lag <= n - 1:
        raise ValueError(f"chain autocorrelation: max_lag must be a whole number in 1..rows - 1 = {n - 1}, got {max_lag}")
    return int(max_lag)


def _chain_first(rows, first):
    if int(first) != first or not 0 <= first <= rows:
        raise ValueError(f"chain autocorrelation: first must be a whole number in 0..rows = {rows}, got {first}")
    return int(first)


def chain_mean(x) -> np.ndarray:
    """The two-pass mean of every series of x[n, ...] over its first axis: m1 = (sum x) / n, m = m1 + (sum (x - m1)) / n, both sums
    sequential in ascending t (vag::chain_mean, to the bit)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m1 = np.cumsum(x, axis=0)[-1] / n
    return m1 + np.cumsum(x - m1, axis=0)[-1] / n


def sokal_window(rho, c: float = 5.0):
    """Sokal's window on rho[L + 1] or rho[L + 1, D]: tau(M) = 2 sum_{l <= M} rho(l) - 1 (sequential), the smallest M with
    M >= c tau(M).  Returns (tau, window): tau(M) at that M, or tau(L) and -1 where there is none (vag::sokal_window, to the bit)."""
    rho = np.asarray(rho, dtype=np.float64)
    flat = rho.reshape(rho.shape[0], -1)
    with np.errstate(invalid="ignore"):
        taus = 2.0 * np.cumsum(flat, axis=0) - 1.0
        ok = np.arange(flat.shape[0], dtype=np.float64)[:, None] >= c * taus
    found = ok.any(axis=0)
    first = np.argmax(ok, axis=0)
    window = np.where(found, first, -1).astype(np.int32)
    tau = np.where(found, taus[first, np.arange(flat.shape[1])], taus[-1])
    return tau.reshape(rho.shape[1:]), window.reshape(rho.shape[1:])


def _chain_record(tau, window, rho, n, L, tol):
    with np.errstate(invalid="ignore"):
        reliable = (window >= 0) & (n >= tol * tau)
    return ChainAutocorr(tau, window, reliable, rho, int(n), int(L))


def chain_autocorr(chain, c: float = 5.0, tol: float = 50.0, max_lag: Optional[int] = None, first: int = 0) -> ChainAutocorr:
    """The integrated autocorrelation time of every parameter of chain[rows, W, D] from row ``first`` on, in numpy, by direct sums (no
    FFT): the two-pass mean of every walker's series, its lag sums c(l) = sum_t y[t] y[t + l] for l = 0 .. L, the sums pooled over the
    walkers (one normalisation for the ensemble, so a walker that never moved adds zeros where emcee's per-walker normalisation gives
    0 / 0), rho = C(l) / C(0) and Sokal's window with constant c.  L is ``max_lag`` or default_max_lag(n, c, tol).  The device estimate
    (chain_autocorr_device) follows the same definition with every lag sum as one fma chain; the two differ by rounding alone."""
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("chain autocorrelation: the chain must be [rows, nwalkers, ndim]")
    first = _chain_first(x.shape[0], first)
    n, W, D = x.shape[0] - first, x.shape[1], x.shape[2]
    L = _chain_lags(n, c, tol, max_lag)
    x = x[first:].reshape(n, W * D)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y = x - chain_mean(x)
        lag = np.empty((L + 1, W * D))
        for l in range(L + 1):
            lag[l] = np.sum(y[:n - l] * y[l:], axis=0)
        pooled = np.cumsum(lag.reshape(L + 1, W, D), axis=1)[:, -1]  # (ascending w)
        rho = pooled / pooled[0]
    tau, window = sokal_window(rho, c)
    bad = ~np.isfinite(pooled[0]) | (pooled[0] == 0.0)
    return _chain_record(np.where(bad, np.nan, tau), np.where(bad, -1, window).astype(np.int32), rho, n, L, tol)


def chain_autocorr_device(chain, c: float = 5.0, tol: float = 50.0, max_lag: Optional[int] = None, first: int = 0, device: int = 0,
                          context=None, rho: bool = True) -> ChainAutocorr:
    """chain_autocorr on a float64 torch tensor [rows, W, D] that lives on GPU ``device`` (vag_chain_autocorr_dev, on torch's current
    stream): the chain is read where it is and only tau, the windows and, with ``rho``, rho come to the host.  A view whose last two
    dimensions are contiguous is taken without a copy -- the cold rung ``chain[:, 0]`` of a tempered chain [rows, T, W, D] for
    instance; anything else is refused.  ``context``: a (handle, lock) pair other than the device's shared context."""
    import ctypes as C
    import torch
    from . import _lib
    from .fitting import on_current_stream
    from .model import get_context
    if not isinstance(chain, torch.Tensor) or chain.dtype != torch.float64 or chain.dim() != 3:
        raise ValueError("chain autocorrelation: the chain must be a float64 torch tensor [rows, nwalkers, ndim]")
    dev = torch.device("cuda", device)
    if chain.device != dev:
        raise ValueError(f"chain autocorrelation: the chain must be on {dev}, it is on {chain.device}")
    rows, W, D = (int(v) for v in chain.shape)
    if W < 1 or D < 1:
        raise ValueError("chain autocorrelation: the chain must be [rows, nwalkers, ndim]")
    first = _chain_first(rows, first)
    n = rows - first
    L = _chain_lags(n, c, tol, max_lag)
    if chain.stride(2) != 1 or chain.stride(1) != D or chain.stride(0) < W * D:
        raise ValueError("chain autocorrelation: the last two dimensions of the chain must be contiguous and the rows must not overlap "
                         f"(strides {tuple(chain.stride())} of shape {tuple(chain.shape)}); make a contiguous copy")
    lib = _lib.load()
    entry = _lib.chain_entry(lib)
    h, lock = get_context(device) if context is None else context
    spec = _lib.ChainSpec(W, D, n, int(chain.stride(0)), L, float(c))
    d_tau = torch.empty((D,), dtype=torch.float64, device=dev)
    d_window = torch.empty((D,), dtype=torch.int32, device=dev)
    d_rho = torch.empty((L + 1, D), dtype=torch.float64, device=dev) if rho else None
    on_current_stream(lib, h, lock, dev, lambda: _lib.check(entry(
        h, C.byref(spec), chain.data_ptr() + 8 * first * int(chain.stride(0)), d_rho.data_ptr() if rho else None, d_tau.data_ptr(),
        d_window.data_ptr())))
    return _chain_record(d_tau.cpu().numpy(), d_window.cpu().numpy(), d_rho.cpu().numpy() if rho else None, n, L, tol)


# ---- posterior-predictive bands (INTEGRATION.md "Posterior-predictive bands"): the quantiles of every column of an array of draws over
#      its valid draws.  The numpy statement first, then the device; Fitter.predict runs the draws' models and this stage in one call. ----

PREDICT_MAX_DRAWS, PREDICT_MAX_Q, PREDICT_MAX_VALUES = 4096, 16, 1 << 27  # VAG_PREDICT_MAX_DRAWS, _Q, _VALUES

Prediction = namedtuple("Prediction", "quantiles bands n_valid valid draw_index t nu draws")
Prediction.__doc__ = """What Fitter.predict returns: the quantile levels [nq], bands[nq, nnu, nt] (NaN throughout when no draw is valid),
the number of valid draws, valid[S], draw_index[S] (the rows of ``samples`` that were drawn, ascending), the grid t[nt] and nu[nnu],
and draws[S, nnu, nt] (None unless asked for; an invalid draw as it came out: NaN where the engine did not evaluate it)."""


def _quantile_levels(q) -> np.ndarray:
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= PREDICT_MAX_Q:
        raise ValueError(f"column quantiles: between 1 and {PREDICT_MAX_Q} quantiles are needed, got shape {q.shape}")
    if not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"column quantiles: every quantile must be in [0, 1], got {q.tolist()}")
    return q


def _quantile_shape(shape):
    """(S, M) of draws [S, ...] with the trailing dimensions as one row of columns, or the refusal."""
    if len(shape) < 2:
        raise ValueError(f"column quantiles: the draws must be [draws, columns] (or [draws, ...]), got shape {tuple(shape)}")
    S, M = int(shape[0]), int(np.prod(shape[1:], dtype=np.int64))
    if S < 1 or M < 1:
        raise ValueError(f"column quantiles: at least one draw and one column are needed, got shape {tuple(shape)}")
    if S > PREDICT_MAX_DRAWS:
        raise ValueError(f"column quantiles: {S} draws exceed the maximum of {PREDICT_MAX_DRAWS}")
    if S * M > PREDICT_MAX_VALUES:
        raise ValueError(f"column quantiles: {S} draws of {M} columns exceed the maximum of {PREDICT_MAX_VALUES} values")
    return S, M


def _exact_fma(g: float, d: float, a: float) -> float:
    """g * d + a with one rounding (std::fma), by exact rational arithmetic."""
    from fractions import Fraction
    if not (math.isfinite(d) and math.isfinite(a)):
        return g * d + a
    try:
        return float(Fraction(g) * Fraction(d) + Fraction(a))
    except OverflowError:
        return math.copysign(math.inf, a)


def quantile_rank(q: float, n: int):
    """(lo, g) of quantile q among n values: h = q * float(n - 1) as one FP64 multiply, lo = floor(h), g = h - lo (vag::predict_rank)."""
    h = float(np.float64(q) * np.float64(n - 1))
    lo = math.floor(h)
    return int(lo), h - lo


def column_quantiles(F, q, valid=None):
    """The quantiles q[nq] of every column of the draws F[S, ...] over the valid draws, in numpy: (Q[nq, ...], valid[S], n_valid).  A
    draw is valid when its flag is set (``valid``, default: all) and all of its values are finite; with n valid draws and y a column's
    valid values in ascending order (np.sort; a zero of either sign read as +0), h = q (n - 1), lo = floor(h), g = h - lo and
    Q = y[lo] where g == 0, else fma(g, y[lo + 1] - y[lo], y[lo]) with the fma evaluated exactly -- numpy's default "linear" quantile
    with the rounding fixed.  No valid draw: Q is NaN.  The device (column_quantiles_device, Fitter.predict) gives the same bits."""
    F = np.asarray(F)
    if F.dtype != np.float64:
        raise ValueError(f"column quantiles: the draws must be float64, got {F.dtype}")
    q = _quantile_levels(q)
    S, M = _quantile_shape(F.shape)
    flat = F.reshape(S, M)
    ok = np.all(np.isfinite(flat), axis=1)
    if valid is not None:
        flags = np.asarray(valid)
        if flags.shape != (S,) or flags.dtype.kind not in "biu":
            raise ValueError(f"column quantiles: valid must be {S} flags (bool or integer), got shape {flags.shape} of {flags.dtype}")
        ok &= flags != 0
    n = int(ok.sum())
    Q = np.full((q.size, M), np.nan)
    if n > 0:
        y = flat[ok]
        y = np.sort(np.where(y == 0.0, 0.0, y), axis=0)
        for k in range(q.size):
            lo, g = quantile_rank(q[k], n)
            Q[k] = y[lo]
            if g != 0.0:
                d = y[lo + 1] - y[lo]
                for m in np.nonzero(d != 0.0)[0]:  # (d == 0: the fma is y[lo])
                    Q[k, m] = _exact_fma(g, float(d[m]), float(y[lo, m]))
    return Q.reshape((q.size,) + F.shape[1:]), ok, n


def column_quantiles_device(F, q, valid=None, device: int = 0, context=None):
    """column_quantiles on a contiguous float64 torch tensor F[S, ...] that lives on GPU ``device`` (vag_column_quantiles_dev, on
    torch's current stream): the draws are read where they are and only Q, the validity and its count come to the host, as numpy
    arrays.  ``valid``: None or S flags (a torch tensor on the device, or anything numpy takes).  ``context``: a (handle, lock) pair
    other than the device's shared context."""
    import ctypes as C
    import torch
    from . import _lib
    from .fitting import on_current_stream
    from .model import get_context
    if not isinstance(F, torch.Tensor) or F.dtype != torch.float64:
        raise ValueError("column quantiles: the draws must be a float64 torch tensor [draws, columns]")
    dev = torch.device("cuda", device)
    q = _quantile_levels(q)
    S, M = _quantile_shape(tuple(F.shape))
    if F.device != dev:
        raise ValueError(f"column quantiles: the draws must be on {dev}, they are on {F.device}")
    if not F.is_contiguous():
        raise ValueError("column quantiles: the draws must be contiguous; make a contiguous copy")
    flags = None
    if valid is not None:
        flags = valid if isinstance(valid, torch.Tensor) else torch.as_tensor(np.asarray(valid))
        if tuple(flags.shape) != (S,) or flags.dtype.is_floating_point or flags.dtype.is_complex:
            raise ValueError(f"column quantiles: valid must be {S} flags (bool or integer), got shape {tuple(flags.shape)} of {flags.dtype}")
        flags = (flags != 0).to(device=dev, dtype=torch.int32).contiguous()
    lib = _lib.load()
    entry = _lib.predict_entry(lib, "vag_column_quantiles_dev")
    h, lock = get_context(device) if context is None else context
    spec = _lib.QuantileSpec(q.size, 0, (C.c_double * 16)(*q.tolist()))
    d_out = torch.empty((q.size, M), dtype=torch.float64, device=dev)
    d_valid = torch.empty((S,), dtype=torch.int32, device=dev)
    d_n = torch.empty((1,), dtype=torch.int32, device=dev)
    on_current_stream(lib, h, lock, dev, lambda: _lib.check(entry(
        h, C.byref(spec), F.data_ptr(), S, M, flags.data_ptr() if flags is not None else None, d_out.data_ptr(), d_valid.data_ptr(),
        d_n.data_ptr())))
    return d_out.cpu().numpy().reshape((q.size,) + tuple(F.shape[1:])), d_valid.cpu().numpy() != 0, int(d_n.cpu().numpy()[0])


def _empty_record(ndim):
    return ChainAutocorr(np.full(ndim, np.nan), np.full(ndim, -1, dtype=np.int32), np.zeros(ndim, dtype=bool), None, 0, 0)


class _ConvergenceMonitor:
    """What the three device run drivers share of ``converge=``: where the chunks end, the estimate at a check, the final record."""

    def __init__(self, converge, nsteps, nburn, thin, chunk, device, cold):
        if converge is not None and not isinstance(converge, Convergence):
            raise ValueError("converge must be a sampling.Convergence or None")
        if int(nburn) != nburn or nburn < 0:
            raise ValueError("nburn must be a whole number of steps >= 0")
        self.rule, self.nsteps, self.first, self.thin, self.chunk = converge, int(nsteps), int(nburn) // thin, thin, chunk
        self.device, self.cold = device, cold  # cold(chain, rows): the view [rows kept so far, W, D] the estimate reads
        self.history, self.previous, self.last, self.last_step, self.converged = [], None, None, -1, False

    def chunk_end(self, step0):
        """The end of the chunk that starts at step0: a check lands after every `check` steps."""
        end = min(step0 + self.chunk, self.nsteps)
        if self.rule is not None:
            end = min(end, (step0 // self.rule.check + 1) * self.rule.check)
        return end

    def estimate(self, chain, step):
        rows = step // self.thin
        rule = self.rule or Convergence()
        if rows - self.first < 2:
            self.last = _empty_record(int(chain.shape[-1]))
        else:
            self.last = chain_autocorr_device(self.cold(chain[:rows]), c=rule.c, tol=rule.tol, first=self.first, device=self.device,
                                              rho=False)
        self.last_step = step
        return self.last

    def stop(self, chain, step):
        """After the chunk that ended at `step`: True when the run ends here."""
        if self.rule is None or step % self.rule.check != 0:
            return False
        rec = self.estimate(chain, step)
        self.history.append(rec.tau.copy())
        self.converged = self.rule.met(rec.tau, rec.reliable, self.previous)
        self.previous = rec.tau
        return self.converged

    def record(self, chain, step):
        if self.last_step != step:
            self.estimate(chain, step)
        ndim = int(chain.shape[-1])
        return ConvergedAutocorr(*self.last, self.converged, int(step), np.array(self.history).reshape(len(self.history), ndim), self.thin)


def _fit_nested(fitter, param_defs, n_live, niter, seed, rng, dlogz, walk, priors):
    """fit(sampler="nested"): the live points from the priors, the run, the evidence."""
    spec, lower, upper = fitter.build_spec(param_defs, priors=priors, use_priors=True)
    ndim = int(spec.ndim)
    walk = nested_default_walk(ndim) if walk is None else walk
    _check_nested(n_live, ndim, walk)
    _nested_stop(dlogz, niter, 1)
    fitter._refuse_host_priors(param_defs, "fit(sampler='nested')")
    prior_specs = list(fitter._prior_specs)
    log_mass = math.log(prior_mass(lower, upper, prior_specs))
    kept, tried, finite = [], 0, 0
    while sum(len(x) for x in kept) < n_live:
        if tried >= 64 * n_live:
            raise ValueError(f"fit(sampler='nested'): {finite} of {tried} prior draws have a finite ln L; no {n_live} live points")
        x = sample_prior(lower, upper, prior_specs, n_live, rng)
        lnl, lnprior = fitter.log_like_and_prior_batch(x, param_defs, priors=priors)
        ok = np.isfinite(lnl) & np.isfinite(lnprior)
        kept.append(x[ok])
        tried, finite = tried + n_live, finite + int(ok.sum())
    live0 = np.concatenate(kept)[:n_live]
    fraction = finite / tried
    run = run_nested_device(fitter, param_defs, live0, niter, walk=walk, seed=seed, dlogz=dlogz, priors=priors)
    ev = nested_evidence(run.dead_lnl, run.lnl)
    samples = np.concatenate([run.dead_theta.reshape(-1, ndim), run.live])
    log_like = np.concatenate([run.dead_lnl.ravel(), run.lnl])
    log_prior = np.concatenate([run.dead_lnprior.ravel(), run.lnprior])
    fraction_err = math.sqrt((1.0 - fraction) / (fraction * tried))  # of ln prior_fraction: the binomial error of the share
    return {"samples": samples, "log_like": log_like, "log_prior": log_prior, "log_weights": ev.log_weights,
            "equal_samples": samples[nested_equal_samples(ev.log_weights, seed)], "best": samples[np.argmax(log_like + log_prior)],
            "log_evidence": ev.ln_z + math.log(fraction), "log_evidence_error": math.hypot(ev.ln_z_err, fraction_err),
            "information": ev.information, "prior_fraction": fraction, "log_prior_mass": log_mass, "niter": run.niter,
            "ncall": tried + run.niter * (n_live // 2) * walk, "acceptance": run.accepted / float((n_live // 2) * walk)}


def fit(fitter: Fitter, param_defs: Sequence[ParamDef], nwalkers: int, nsteps: int, nburn: int = 0, seed: int = 0,
        loglike_fn: Optional[Callable] = None, center: Optional[np.ndarray] = None, spread: float = 0.1, sampler: str = "host",
        ntemps: int = 8, beta_min: float = 1e-3, prior_rung: bool = True, moves=None, converge: Optional[Convergence] = None,
        dlogz: float = 0.1, walk: Optional[int] = None, priors=None):
    """Convenience driver: uniform priors over the ParamDef boxes, stretch-move sampling on the device likelihood.
    Returns dict(samples[flat, ndim], log_prob[flat], acceptance, best) in sampler space (log10 for LOG parameters).
    ``sampler="host"``: run_stretch_move in numpy around one device call per half-step; ``"device"``: run_stretch_move_device, the
    whole run on the device (fixed halves and Philox draws keyed by `seed`: another chain than the host sampler's, the same
    distribution) -- with ``moves=None`` the stretch move, with ``moves="reference"`` (REFERENCE_MOVES: the DE move at 0.8 and the
    snooker move at 0.2, the reference's own mix) or a sequence of (name, weight) over MOVE_KINDS run_moves_device; ``"tempered"``: run_tempered_device on the ladder geometric_betas(ntemps, beta_min, prior_rung), `nwalkers` per
    temperature.  The keys above are then filled from the cold chain (beta = 1, log_prob = ln L + ln prior), and the dict also holds
    "betas", "log_like" (the mean of ln L per rung after the burn-in), "log_evidence" and "log_evidence_error"
    (thermodynamic_evidence of those means: read its caveats) and "swap_fraction".

    Every sampler also returns "tau" (the integrated autocorrelation time of each parameter over the rows after `nburn`, in steps;
    NaN when fewer than two rows are kept) and "tau_reliable" (a window was found and the kept rows number at least 50 tau, or
    ``converge.tol`` tau): the device samplers from chain_autocorr_device on the chain in HBM ("tempered": the cold rung), the host
    sampler from chain_autocorr.  ``converge=Convergence(...)`` (device samplers only) makes `nsteps` a maximum and stops the run by
    that rule (run_stretch_move_device); the dict then also holds "converged" and "nsteps", the steps run.

    ``sampler="nested"``: nested sampling on the device (run_nested_device) with `nwalkers` live points, `nsteps` the maximum number
    of iterations, stopped by ``dlogz`` (nested_remaining), ``walk`` constrained steps per iteration (None: max(20, 5 ndim)) and the
    priors ``priors`` (as Fitter.log_prob_batch takes them; device-evaluated ones only; None: uniform over the boxes).  The live points
    are drawn from the priors inside the boxes (sample_prior) in batches through Fitter.log_like_and_prior_batch; the first `nwalkers`
    with finite ln L are kept and "prior_fraction" is the share of all points tried whose ln L was finite.  The dict holds "samples"
    (the dead points in the order they were retired, then the final live points) with "log_like", "log_prior" and the normalised
    "log_weights", "equal_samples" (nested_equal_samples), "best" (the sample of highest ln L + ln prior), "log_evidence",
    "log_evidence_error", "information", "prior_fraction", "log_prior_mass", "niter", "ncall" (the points tried included) and
    "acceptance" (per iteration).  "log_evidence" includes ln prior_fraction: the points where the model does not evaluate count as
    L = 0.  The tempered number excludes it: its beta = 0 rung is the prior restricted to where the model evaluates.  Both are
    relative to the prior mass inside the boxes, returned here as "log_prior_mass" (prior_mass): the integral of L times the prior
    density over the boxes is exp(log_evidence + log_prior_mass).  "log_evidence_error" is sqrt(H / N) and the binomial error of
    ln prior_fraction in quadrature."""
    if sampler not in ("host", "device", "tempered", "nested"):
        raise ValueError(f"unknown sampler {sampler!r}: 'host', 'device', 'tempered' or 'nested'")
    if converge is not None and sampler == "host":
        raise ValueError("converge stops a run on the device: sampler='host' runs its fixed nsteps (sampler='device' or 'tempered')")
    if converge is not None and sampler == "nested":
        raise ValueError("converge stops a run by its autocorrelation times: sampler='nested' has no chain and stops by dlogz "
                         "(sampler='device' or 'tempered')")
    if priors is not None and sampler != "nested":
        raise ValueError(f"priors shapes the live points and the evidence of sampler='nested'; sampler={sampler!r} samples uniform priors "
                         "over the boxes (compose the run drivers, which take priors, instead)")
    if converge is not None and not isinstance(converge, Convergence):
        raise ValueError("converge must be a sampling.Convergence or None")

    def tau_keys(rec, thin=1):
        keys = {"tau": rec.tau * thin, "tau_reliable": rec.reliable}
        if converge is not None:
            keys.update(converged=rec.converged, nsteps=rec.steps)
        return keys
    if sampler != "host" and loglike_fn is not None:
        raise ValueError(f"sampler={sampler!r} evaluates the fitter's own likelihood on the device: it cannot be combined with "
                         "loglike_fn (compose sampling.StretchMove or sampling.TemperedMove with your evaluator instead)")
    if moves is not None and sampler != "device":
        raise ValueError(f"moves selects the proposals of sampler='device'; sampler={sampler!r} knows the stretch move alone "
                         "(compose sampling.EnsembleMoves with your evaluator instead)")
    if moves is not None:
        move_weights(moves)  # (refused before anything is built)
    rng = np.random.default_rng(seed)
    if sampler == "nested":
        return _fit_nested(fitter, param_defs, int(nwalkers), int(nsteps), seed, rng, dlogz, walk, priors)
    if sampler == "tempered":
        betas = geometric_betas(ntemps, beta_min, prior_rung)
        _, lower, upper = fitter.build_spec(param_defs)
        pos0 = initial_positions(lower, upper, betas.size * nwalkers, rng, center=center, spread=spread).reshape(betas.size, nwalkers, -1)
        chain, lnl, lnprior, acc, swap_fraction, rec = run_tempered_device(fitter, param_defs, pos0, betas, nsteps, seed=seed,
                                                                           converge=converge, nburn=max(int(nburn), 0), _record=True)
        cold, logp = chain[:, 0], lnl[:, 0] + lnprior[:, 0]
        flat = cold[nburn:].reshape(-1, cold.shape[-1])
        flat_lp = logp[nburn:].reshape(-1)
        log_like = lnl[nburn:].mean(axis=(0, 2)) if lnl[nburn:].size else np.full(betas.size, np.nan)
        ln_z, ln_z_err = thermodynamic_evidence(betas, log_like)
        return {"samples": flat, "log_prob": flat_lp, "acceptance": acc[0], "best": flat[np.argmax(flat_lp)], "chain": cold,
                "betas": betas, "log_like": log_like, "log_evidence": ln_z, "log_evidence_error": ln_z_err,
                "swap_fraction": swap_fraction, **tau_keys(rec)}
    _, lower, upper = fitter.build_spec(param_defs)
    if sampler == "device":
        pos0 = initial_positions(lower, upper, nwalkers, rng, center=center, spread=spread)
        if moves is None:
            chain, logp, acc, rec = run_stretch_move_device(fitter, param_defs, pos0, nsteps, seed=seed, converge=converge,
                                                            nburn=max(int(nburn), 0), _record=True)
        else:
            chain, logp, acc, rec = run_moves_device(fitter, param_defs, pos0, nsteps, moves=moves, seed=seed, converge=converge,
                                                     nburn=max(int(nburn), 0), _record=True)
    else:
        log_prob_batch = fitter.make_log_prob_batch(param_defs, loglike_fn=loglike_fn)
        pos0 = initial_positions(lower, upper, nwalkers, rng, center=center, spread=spread)
        chain, logp, acc = run_stretch_move(log_prob_batch, pos0, nsteps, rng=rng)
        kept = chain.shape[0] - min(max(int(nburn), 0), chain.shape[0])
        rec = chain_autocorr(chain, first=chain.shape[0] - kept) if kept >= 2 else _empty_record(chain.shape[-1])
    flat = chain[nburn:].reshape(-1, chain.shape[-1])
    flat_lp = logp[nburn:].reshape(-1)
    return {"samples": flat, "log_prob": flat_lp, "acceptance": acc, "best": flat[np.argmax(flat_lp)], "chain": chain, **tau_keys(rec)}
