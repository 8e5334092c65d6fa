"""The split flux kernel's instruction forms of exp2_fast and sp_fast<true> (vag_device.h: exp2_fast_as with the first Horner step
as one v_fma_f64 and the nine scalar-addend steps in one asm statement, sp_fast with its magic number in a vector register; DESIGN
4g item 14) against the forms the rest of the library keeps, on the device through vag_debug_device_math, bit for bit
(np.array_equal on the words, so NaN compares by its bits too).  The existing functions are the reference;
tests/test_device_math.py holds them to high precision.  exp2_or_zero keeps its one form: the one-statement chain lost on the
interpolation team (profiles/flux_chain_ab.txt) and is not in the tree; its arguments [-1100, 1100], -2000 and the clamp's image of
-inf and NaN are exp2_fast arguments here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def dev():
    from vegasafterglow_amd import _lib
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    ids = {**_lib.MATH, **_lib.MATH_MORE}

    def run(name, x, n_out=1):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.full((x.shape[0], n_out), np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, ids[name], x.ctypes.data_as(_dp), x.shape[0], out.ctypes.data_as(_dp)))
        return out if n_out > 1 else out[:, 0]
    yield run
    lib.vag_ctx_destroy(ctx)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def neighbours(x, k=3):
    out = [np.asarray(x, dtype=np.float64)]
    for to in (np.inf, -np.inf):
        y = out[0]
        for _ in range(k):
            y = np.nextafter(y, to)
            out.append(y)
    return np.concatenate(out)


def exp2_points():
    rng = np.random.default_rng(5)
    halves = np.arange(-2200, 2201) * 0.5  # every integer and every tie of the round-to-nearest split in [-1100, 1100]
    return np.concatenate([np.linspace(-1100, 1100, 100001), rng.uniform(-1100, 1100, 20000), rng.uniform(-1, 1, 5000),
                           neighbours(halves), np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300])])


def test_exp2_fast_chain_has_the_bits_of_exp2_fast(dev):
    x = np.concatenate([exp2_points(), neighbours(np.array([-2000.0])), np.array([-2000.0, 2000.0])])  # -2000: exp2_or_zero's clamp
    ref = dev("exp2_fast", x)
    assert ref[-2] == 0 and np.isinf(ref[-1])
    assert same_bits(dev("exp2_fast_chain", x), ref)


def test_sp_fast_with_the_magic_number_in_a_register_has_the_bits_of_sp_fast(dev):
    z = np.concatenate([np.linspace(-21, 21, 100001), neighbours(np.array([0.0, -0.0, 20.0, -20.0])),
                        neighbours(np.arange(-200, 201) * 0.1), neighbours(np.arange(-400, 401) * 0.05),  # nodes, interval edges
                        np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, 5e-324, -5e-324])])
    ref = dev("sp_fast_relu", z)
    assert same_bits(dev("sp_fast_relu_vmagic", z), ref)
    # sp_fast<true> against the plain form (equal as numbers: the relu form gives max(z, 0) = +0 where the plain form may give -0)
    plain = dev("sp_fast", z)
    ok = np.isfinite(plain)
    assert np.array_equal(ref[ok], plain[ok]) and np.array_equal(np.isnan(ref), np.isnan(plain))
