"""The split form of the headline flux pass (vag_flux_grid_split_kernel: some wavefronts of a workgroup compute the boundary spectra
of the next row while the others interpolate the present one into accumulators they keep in registers, one barrier per row) gives
every (nu, t) sum the addends of the present kernel in the same row order: every result must be bit-for-bit the one of
VAG_FLUX_SPLIT=0.  The product takes the split form only where it is measured to win; the small cases here force it
(VAG_FLUX_SPLIT=2, on a persistent launch: VAG_FLUX_PERSISTENT=2; VAG_FLUX_WIDE keeps the 512-lane workgroups on small grids)."""
import ctypes as C
import re

import numpy as np
import pytest

import _abi
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

M12 = (0.2, 0.7, 12.0)   # ~36 phi rows per theta row
R5 = (0.3, 1.0, 5.0)     # ~54 phi rows; lattices of ~50 / ~100 / ~200 nodes: at ten frequencies 250 / 500 / 1000 boundary work
R10 = (0.3, 1.0, 10.0)   # items, below and above the lanes of any boundary team
R20 = (0.3, 1.0, 20.5)
NU10 = configs.C2_NU
NU = {1: np.array([4.84e14]), 3: np.array([1e9, 4.84e14, 1e18]), 10: NU10}


@pytest.fixture(scope="module")
def eng():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    h, lock = va.get_context(0)
    return lib, h


def grid(eng, prms, t, nu, ok_rc=()):
    lib, h = eng
    arr = (_lib.ModelParams * len(prms))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in prms])
    t = np.ascontiguousarray(t, dtype=np.float64)
    nu = np.ascontiguousarray(nu, dtype=np.float64)
    out = np.empty((len(prms), nu.size, t.size))
    rc = lib.vag_flux_density_grid_batch(h, arr, len(prms), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                         out.ctypes.data_as(dp))
    if rc not in ok_rc:
        _lib.check(rc)
    return out, rc


def jittered(kw0, nb, seed):
    """bench.py's batch: +-10 % log-uniform jitter of the physical parameters (seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nb):
        kw = dict(kw0)
        j = lambda: float(np.exp(rng.uniform(np.log(0.9), np.log(1.1))))
        for name in ("E_iso", "Gamma0", "n_ism", "eps_e", "eps_B", "theta_c"):
            if name in kw:
                kw[name] *= j()
        kw["p"] = kw.get("p", 2.3) + rng.uniform(-0.1, 0.1)
        out.append(_abi.make_params(**kw))
    return out


def c2(res, nb, seed, **kw):
    return jittered(dict(configs.C2, resolutions=res, **kw), nb, seed)


def scramble(eng):
    """A call of another shape, so that neither run finds partial grids of its own shape left in the context's buffers (an item a
    launch skipped would then read as garbage, not as the other run's value)."""
    grid(eng, c2(M12, 3, 99), np.logspace(3, 7, 13), np.array([1e10, 1e15]))


def run_form(eng, capfd, split, prms, t, nu, extra=None, force=True, ok_rc=()):
    """One call under VAG_FLUX_SPLIT=split; asserts from the launch report which form ran.  Returns (fluxes, rc, report)."""
    hooks = dict(extra or {})
    hooks.update({"VAG_DEBUG_LAUNCH": "1", "VAG_FLUX_WIDE": "1"})
    if force:
        hooks["VAG_FLUX_PERSISTENT"] = "2"
    if split is not None:
        hooks["VAG_FLUX_SPLIT"] = str(split)
    for k, v in hooks.items():
        _lib.hooks[k] = v
    try:
        scramble(eng)
        capfd.readouterr()
        out, rc = grid(eng, prms, t, nu, ok_rc)
        err = capfd.readouterr().err
    finally:
        for k in hooks:
            _lib.hooks.pop(k, None)
    assert "grid flux form: persistent" in err and "grid flux form: one item" not in err, err
    if split == 0:
        assert "grid flux split:" not in err, err
    else:
        assert "grid flux split:" in err, err
    return out, rc, err


def both(eng, capfd, prms, t, nu, extra=None, **kw):
    new = run_form(eng, capfd, 2, prms, t, nu, extra, **kw)
    old = run_form(eng, capfd, 0, prms, t, nu, extra, **kw)
    return new[0], old[0]


def assert_bits(new, old):
    assert np.all(np.isfinite(new)) and new.max() > 0
    assert np.array_equal(new, old)


@pytest.fixture(scope="module")
def b_lanes(eng):
    """Lanes of the interpolation team, from the launch report of a forced split call (the team sizes are the library's)."""
    hooks = {"VAG_DEBUG_LAUNCH": "1", "VAG_FLUX_WIDE": "1", "VAG_FLUX_PERSISTENT": "2", "VAG_FLUX_SPLIT": "2"}
    import os
    import tempfile
    for k, v in hooks.items():
        _lib.hooks[k] = v
    # the report goes to the C stderr: capture file descriptor 2 around the call
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            grid(eng, c2(M12, 1, 1), np.logspace(3, 7, 9), NU[3])
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            for k in hooks:
                _lib.hooks.pop(k, None)
        f.seek(0)
        err = f.read().decode()
    m = re.search(r"grid flux split: (\d+) \+ (\d+) wavefronts", err)
    assert m, err
    assert int(m.group(1)) + int(m.group(2)) == 8
    return 64 * int(m.group(2))


@pytest.fixture(scope="module")
def prms_r10():
    return c2(R10, 2, 21)


@pytest.mark.parametrize("nnu", [1, 3, 10])
@pytest.mark.parametrize("nt_kind", ["one", "team", "team_plus_one", "bench"])
def test_grid_shapes_around_the_ownership_of_times(eng, capfd, b_lanes, prms_r10, nt_kind, nnu):
    """nt = 1, the interpolation team's lanes (every lane one time), one more (the first lane a second time) and 200; one frequency,
    three (odd: the duplicated last pair of the boundary items) and ten."""
    nt = {"one": 1, "team": b_lanes, "team_plus_one": b_lanes + 1, "bench": 200}[nt_kind]
    t = np.array([3e5]) if nt == 1 else np.logspace(2, 8, nt)
    new, old = both(eng, capfd, prms_r10, t, NU[nnu])
    assert_bits(new, old)


@pytest.mark.parametrize("res,ppb", [(R5, 1), (R10, 2), (R5, 57), (M12, 39), (R20, 50)])
def test_items_and_pipeline_edges(eng, capfd, res, ppb):
    """Items of one row (the pipeline fills and drains with nothing between), of two rows, of a whole theta row plus three (~54 and
    ~36 phi rows: the re-staging falls inside an item, at a place that moves from item to item), and a last item shorter than the
    others (50 rows per item)."""
    new, old = both(eng, capfd, c2(res, 2, 31 + ppb), np.logspace(2.5, 7.5, 37), NU10, {"VAG_PAIRS_PER_BLOCK": str(ppb)})
    assert_bits(new, old)


@pytest.mark.parametrize("ppb", [1, 7])
def test_on_axis_every_row_restages(eng, capfd, ppb):
    """theta_obs = 0: one phi row per theta row, so every row of an item stages a new photon block."""
    new, old = both(eng, capfd, c2(R10, 3, 41, theta_obs=0.0), np.logspace(2.5, 7.5, 40), NU[3], {"VAG_PAIRS_PER_BLOCK": str(ppb)})
    assert_bits(new, old)


def test_window_that_leaves_the_early_rows_out(eng, capfd):
    new, old = both(eng, capfd, c2(R10, 2, 51), np.logspace(7.5, 8, 5), NU10)
    assert_bits(new, old)


def test_window_at_the_lattices_first_nodes(eng, capfd):
    """Requested times of 1e-30 s.  The grid stage starts every lattice from the first requested time, so no request leaves all rows
    out (probed: on- and off-axis jets from 1e-30 to 1e15 s all give positive fluxes): this is the nearest one, every time
    inside the first interval or before the row.  Fluxes of 1e-129 and below, the same bits in both forms."""
    new, old = both(eng, capfd, c2(R10, 2, 52), np.logspace(-30, -29, 5), NU[3])
    assert_bits(new, old)


def test_mixed_batch_with_a_rejected_model(eng, capfd):
    """A ragged mix of resolutions (the cost order is not the model order) with a model the grid stage rejects (status != 0: its
    items return at once) between good ones."""
    prms = []
    for i, res in enumerate([R10, (0.15, 0.5, 10.0), R20, (0.2, 2.0, 5.0)] * 3):
        prms += c2(res, 1, 60 + i)
    bad = _abi.make_params(**dict(configs.C2, resolutions=(200.0, 0.31, 5.0)))  # 72 000 phi nodes: beyond the grid kernel's layouts
    prms.insert(5, bad)
    t, nu = np.logspace(2.5, 7.5, 37), NU10
    cap = {rc for rc in range(-64, 65) if rc != 0}  # the call reports the rejected model after it has written the others
    new, rc_new, _ = run_form(eng, capfd, 2, prms, t, nu, ok_rc=cap)
    old, rc_old, _ = run_form(eng, capfd, 0, prms, t, nu, ok_rc=cap)
    assert rc_new == rc_old and rc_new != 0
    good = [i for i in range(len(prms)) if i != 5]
    assert_bits(new[good], old[good])


def test_same_call_twice_gives_the_same_bits(eng, capfd):
    prms = c2(R20, 4, 71)
    a = run_form(eng, capfd, 2, prms, configs.C2_T, NU10)[0]
    b = run_form(eng, capfd, 2, prms, configs.C2_T, NU10)[0]
    assert_bits(a, b)


def test_bench_batch_takes_the_split_form_and_is_bitwise_unchanged(eng, capfd):
    """The product's own choice: the bench batch takes the split form without being forced."""
    prms = jittered(configs.C2, 512, seed=0)
    hooks = {"VAG_DEBUG_LAUNCH": "1"}
    res = []
    for split in (None, "0"):
        if split is not None:
            hooks["VAG_FLUX_SPLIT"] = split
        for k, v in hooks.items():
            _lib.hooks[k] = v
        try:
            scramble(eng)
            capfd.readouterr()
            res.append(grid(eng, prms, configs.C2_T, configs.C2_NU)[0])
            err = capfd.readouterr().err
        finally:
            for k in hooks:
                _lib.hooks.pop(k, None)
        assert "grid flux form: persistent" in err and ("grid flux split:" in err) == (split is None), err
    assert_bits(res[0], res[1])
