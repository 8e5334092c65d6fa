"""The inverse-Compton routines on the device against the extended-precision reference of that code alone (tests/_icref.py): the
Klein-Nishina table of the context and its two look-ups, ic_table_eval_hdr, power_law_bin_integral, suffix_scan4, electron_column_den,
IcY, one pass of the gamma_c and gamma_M fixed points, the loops themselves, syn_gamma_a_ic and determine_regime, each through its probe
routine (vag_debug_device_math) on the probe set tests/test_ic_state_host.py shows a float64 restatement to meet the ceilings on.
vag_ic_photon_kernel's body, the plan and band kernels stay held end to end (tests/test_gpu_parity.py, tests/test_ic_diagonal_identity.py).

Metric: the relative error of the returned value under the nearest reference the thresholds admit, per quantity and class.  Gates:
GATE_FACTOR x the maxima measured on an MI355X (MEASURED below), each of which must itself stay under its ceiling (_icref.ceiling: 25 x
what IEEE double gives on the formula).  A figure that is missing has not been measured: its test fails after printing it.  Outputs that
are integers, bits, zeros, infinities or a value handed through are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import _icref as R
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")
_dp = C.POINTER(C.c_double)

GATE_FACTOR = 4  # the suite's convention (tests/test_electron_stage.py)
# (quantity, class ...) -> the maximum over the probe set, measured on an MI355X on 2026-10-21, rounded up to two digits
MEASURED = {
    ('lut.ratio',): 2.5e-12, ('lut.lg2_ratio',): 9.3e-11, ('lg2.corr', 'below'): 7.9e-17, ('lg2.corr', 'table'): 2.5e-12,
    ('lg2.corr', 'above'): 1.4e-15, ('lg2.lg2_corr', 'below'): 1.5e-15, ('lg2.lg2_corr', 'table'): 9.3e-11,
    ('lg2.lg2_corr', 'above'): 3.7e-16, ('node.corr', 'below'): 7.9e-17, ('node.corr', 'table'): 2.5e-12,
    ('node.corr', 'above'): 1.5e-15, ('node.lg2_corr', 'below'): 1.5e-15, ('node.lg2_corr', 'table'): 9.3e-11,
    ('node.lg2_corr', 'above'): 3.7e-16, ('table.value',): 8.8e-16, ('bin', 'series'): 2.1e-16, ('bin', 's1~1e-3'): 3.9e-16,
    ('bin', 's1<1e-2'): 1.4e-12, ('bin', 's1<1e-1'): 1.4e-13, ('bin', 's1>=1e-1'): 1.4e-14, ('scan',): 4.3e-16,
    ('column_den', 'slow'): 2.1e-14, ('column_den', 'fast'): 2.0e-14, ('icy.gamma_m_hat',): 3.3e-16, ('icy.gamma_c_hat',): 6.6e-15,
    ('icy.gamma_self',): 2.2e-15, ('icy.slope',): 5.6e-17, ('icy.lg2_lower',): 7.9e-15, ('icy.lg2_const',): 9.7e-16,
    ('icy.Y',): 7.4e-15, ('icy.Y_nu',): 8.1e-15, ('step.Y_T', 'Y_T<1e-3'): 4.5e-13, ('step.Y_T', 'Y_T<1e-4'): 6.1e-12,
    ('step.Y_T', 'Y_T<1e-5'): 5.0e-11, ('step.Y_T', 'Y_T<1e-6'): 5.2e-10, ('step.Y_T', 'Y_T<1e-7'): 3.2e-09,
    ('step.Y_T', 'Y_T<1e-8'): 4.2e-08, ('step.Y_T', 'Y_T>=1e-3'): 7.4e-14, ('step.Y', 'Y_T<1e-3'): 4.5e-13,
    ('step.Y', 'Y_T<1e-4'): 6.1e-12, ('step.Y', 'Y_T<1e-5'): 5.0e-11, ('step.Y', 'Y_T<1e-6'): 5.2e-10, ('step.Y', 'Y_T<1e-7'): 3.2e-09,
    ('step.Y', 'Y_T<1e-8'): 4.2e-08, ('step.Y', 'Y_T>=1e-3'): 7.4e-14, ('step.gc_new',): 2.4e-15, ('step.gM',): 2.1e-15,
    ('step.gM_pass',): 1.6e-15, ('fixed.gc',): 3.5e-15, ('fixed.gc_used',): 7.7e-15, ('fixed.gM',): 4.0e-15, ('ga.gamma_a',): 8.0e-15,
    ('ga.Y_c',): 6.1e-15, ('fixed.Y_T', 'Y_T<1e-3'): 6.2e-13, ('fixed.Y_T', 'Y_T<1e-4'): 7.5e-12, ('fixed.Y_T', 'Y_T<1e-5'): 5.5e-11,
    ('fixed.Y_T', 'Y_T<1e-6'): 5.2e-10, ('fixed.Y_T', 'Y_T<1e-7'): 4.0e-09, ('fixed.Y_T', 'Y_T<1e-8'): 5.2e-08,
    ('fixed.Y_T', 'Y_T<1e-9'): 3.2e-07, ('fixed.Y_T', 'Y_T<1e-10'): 8.8e-07, ('fixed.Y_T', 'Y_T<1e-11'): 1.4e-05,
    ('fixed.Y_T', 'Y_T<1e-12'): 1.7e-04, ('fixed.Y_T', 'Y_T>=1e-3'): 7.0e-14,
}
TABLE = []
NAMES = list(R._MAKERS)


@pytest.fixture(scope="module")
def dev():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    cache = {}

    def run(name, rows=None):
        """The probe routine on rows (default: its probe set, evaluated once)."""
        if rows is None and name in cache:
            return cache[name]
        x = np.ascontiguousarray(R.probe_set(name)[0] if rows is None else rows, dtype=np.float64)
        n_in, n_out = _lib.MATH_IC_SHAPES[name]
        assert x.shape[1] == n_in
        out = np.full((x.shape[0], n_out), np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH_MORE[name], x.ctypes.data_as(_dp), x.shape[0], out.ctypes.data_as(_dp)))
        if rows is None:
            cache[name] = out
        return out
    yield run
    lib.vag_ctx_destroy(ctx)
    if TABLE:
        print("\n[ic state] quantity, class                      measured   gate      ceiling")
        for key, err, gate, ceil in TABLE:
            print(f"[ic state] {' '.join(key):34s} {err:9.2e}  {gate if gate is None else format(gate, '.2e')}  {ceil:.1e}")


def hold(worst):
    """Every measured maximum against its ceiling and its gate; reports all before it fails on any."""
    bad = []
    for key, err in sorted(worst.items()):
        m = MEASURED.get(key)
        ceil = R.ceiling(*key)
        gate = None if m is None else GATE_FACTOR * m
        TABLE.append((key, err, gate, ceil))
        print(f"[ic state] {' '.join(key):34s} measured {err:.3e}  gate {gate}  ceiling {ceil:.1e}")
        if not err <= ceil:
            bad.append(f"{key}: {err:.3e} is above the ceiling {ceil:g}: the device is wrong or the reference is")
        elif m is None:
            bad.append(f"{key}: measured {err:.3e}, no constant recorded")
        elif not (gate <= ceil and err <= gate):
            bad.append(f"{key}: {err:.3e} > {gate:.3e}, or the gate is above the ceiling {ceil:.1e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", NAMES)
def test_probe_routine_against_the_reference(dev, name):
    out = dev(name)
    assert not np.isnan(out).any(), "a probe row gives NaN"
    worst, counts = R.errors(name, out)  # (an output that is not finite is an error unless the reference is that infinity, exactly)
    assert not any(counts.values()), counts
    hold(worst)


def test_the_two_look_ups_agree(dev):
    """compton_correction_pair_lg2 and _node on the same log2 x (the rows whose second column is NaN): bit for bit inside the table, where
    both do the same two multiply-adds on the same words; within the sum of their ceilings in the tails, where one forms 1 / x as 2^-log2 x
    and the other as a reciprocal."""
    rows, kind = R.probe_set("kn_corr")
    out = dev("kn_corr")
    own = np.isnan(rows[:, 1])
    cls = R.kn_class(rows[:, 0] + R.LG2_X_PER_NU)
    inside = own & (cls == "table") & (kind == "random")
    assert inside.sum() >= 1000
    assert np.array_equal(out[inside, 0], out[inside, 2]) and np.array_equal(out[inside, 1], out[inside, 3])
    for c in ("below", "above"):
        sel = own & (cls == c) & np.isfinite(out[:, 1])
        for j, q in ((0, "corr"), (1, "lg2_corr")):
            e = R.rel(out[sel, j], R.ld(out[sel, j + 2])).max()
            bound = R.ceiling("lg2." + q, c) + R.ceiling("node." + q, c)
            print(f"[ic state] |lg2 form - node form| {q:8s} {c:5s} {e:.2e}  bound {bound:.1e}")
            assert e <= bound


@pytest.mark.parametrize("kn", [False, True])
def test_cooling_kernel_writes_an_admitted_iterate_of_every_cell(kn):
    """Ties the probe's function to what vag_ic_cooling_kernel writes: for every cell k >= 1 of every representative row of a small
    forward-shock SSC model, gamma_c[k] of Model.details is within the gc ceiling of a stopping iterate the rule admits for the
    long-double iteration started from the device's own gamma_c[k - 1].  Assumes, unchecked, that these details are the ones an SSC
    model builds after IC cooling.  Cell 0 starts from its synchrotron-only gamma_c, which the details no longer hold: skipped, alone."""
    import _abi
    import _elecref as er
    import _mathref as mr
    import vegasafterglow_amd as va
    prm = _abi.make_params(jet="GaussianJet", theta_obs=0.2, ssc=True, kn=kn, resolutions=(0.06, 0.2, 5.0))
    d = va.Model.from_params(prm).details(1e2, 1e7)
    t, B, gm, gc = d["t_comv"] * mr.U_SEC, d["B"] * er.U_GAUSS, d["gamma_m"], d["gamma_c"]
    assert gc.ndim == 2 and gc.shape[1] >= 8 and gc.shape[0] >= 2 and np.all(np.isfinite(gc)) and np.all(B > 0)
    err, guard = R.chain_errors(t, B, gm, gc, prm.p, prm.eps_e / prm.eps_B, kn)
    assert err.shape == (gc.shape[0], gc.shape[1] - 1) and not guard.any()  # every cell but each row's first
    print(f"[ic state] chain {'KN' if kn else 'Thomson'}: {err.size} cells of {gc.shape[0]} rows, worst {err.max():.2e}, ceiling {R.ceiling('fixed.gc'):.1e}")
    assert err.max() <= R.ceiling("fixed.gc")


@pytest.mark.parametrize("n", [1, 63, 65])
def test_probe_gives_the_same_bits_whatever_the_launch(dev, n):
    for name in NAMES:
        rows, full = R.probe_set(name)[0], dev(name)
        m = 64 * n if name == "ic_suffix_scan" else n  # (a wave routine: whole wavefronts)
        m = min(m, rows.shape[0])
        assert np.array_equal(dev(name, rows[:m]), full[:m], equal_nan=True) and np.array_equal(dev(name, rows[-m:]), full[-m:], equal_nan=True), name
