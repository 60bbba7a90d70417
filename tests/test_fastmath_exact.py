"""The short exact square root and division of csrc/fastmath.h (gs_sqrt_fast, gs_sqrt_core, gs_div_fast), compiled for the host and
compared BIT FOR BIT with sqrt and true division.  They are the refinement cores of the compiler's own expansions without the
scaling frame, so on their domains there is one right answer per input: the correctly rounded one.

The hardware estimates (v_rsq_f64, v_rcp_f64) are stood in for by the true 1 / sqrt(x) and 1 / b cut to 26 significant bits and moved
by -1, 0 or +1 unit of that place, drawn from a seeded generator (tests/native/fastmath_exact_host.cpp): the refinement has to be
right from any estimate of that accuracy.  (No document shipped with the toolchain states a tighter figure for the two instructions.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20                                    # random points per function (>= 10^6)
TINY = 2.0 ** -767                             # below it the compiler's sqrt scales its operand: the core's lower end


def _build(tmp, src, name):
    out = tmp / name
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-I", os.path.join(ROOT, "grid_fed_rl_gym_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", src), "-o", str(out)], check=True)
    return ctypes.CDLL(str(out))


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fastmath_exact")
    lib = _build(tmp, "fastmath_exact_host.cpp", "libfastmath_exact_host.so")
    dp = ctypes.POINTER(ctypes.c_double)
    lib.fx_seed.argtypes = [ctypes.c_uint64]
    for f in (lib.fx_sqrt_fast, lib.fx_sqrt_core, lib.fx_log01):
        f.argtypes = [dp, dp, ctypes.c_long]
    lib.fx_div_fast.argtypes = [dp, dp, dp, ctypes.c_long]
    lib.fx_unit32.argtypes = [ctypes.POINTER(ctypes.c_uint32), dp, dp, ctypes.c_long]
    # the build tests/test_fastmath.py uses: estimates = the true quotients (its gs_log01 is the reference for seed independence)
    plain = _build(tmp, "fastmath_host.cpp", "libfastmath_host.so")
    plain.fm_log01.argtypes = [dp, dp, ctypes.c_long]
    lib.plain = plain
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _call1(f, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    f(_p(x), _p(out), len(x))
    return out


def _div(fx, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    fx.fx_div_fast(_p(a), _p(b), _p(out), len(a))
    return out


def _same_bits(got, ref):
    """Equal bit patterns; a NaN matches any NaN (the payload is not part of the contract)."""
    return (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))


def _log_uniform(rng, lo, hi, n):
    """n doubles whose base-2 logarithm is uniform over [log2 lo, log2 hi] (exponent and mantissa drawn apart: exp() would overflow)."""
    e = rng.uniform(np.log2(lo), np.log2(hi), n)
    k = np.floor(e)
    return np.clip(np.ldexp(np.exp2(e - k), k.astype(np.int64)), lo, hi)


def _neighbours(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)])


def _binade_ends():
    k = np.arange(-40, 41)
    return np.concatenate([np.ldexp(1.0, k), np.nextafter(np.ldexp(1.0, k + 1), 0.0)])


def _radius_arguments(fx):
    """-2 ln u of the first and the last uniform (r + 1/2) 2^-32, through the header's own logarithm."""
    u = (np.array([0.0, 2.0 ** 32 - 1.0]) + 0.5) / 4294967296.0
    return -2.0 * _call1(fx.fx_log01, u)


def test_square_root_equals_sqrt_on_a_million_points_and_every_named_case(fx):
    rng = np.random.default_rng(10)
    squares = np.concatenate([np.arange(1.0, 200.0) ** 2, (rng.integers(1, 1 << 26, 2000).astype(np.float64)) ** 2])
    named = np.concatenate([
        _neighbours(squares), _neighbours(_binade_ends()), _neighbours([TINY]),
        [0.0, -0.0, 5e-324, 2.0 ** -1050, np.inf, np.nan, -1.0, np.finfo(np.float64).max, np.finfo(np.float64).tiny],
        _radius_arguments(fx)])
    x = np.concatenate([_log_uniform(rng, TINY, np.finfo(np.float64).max, N), _log_uniform(rng, 5e-324, TINY, 1 << 16), named])
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(x)
    for seed in (1, 2, 3):
        fx.fx_seed(seed)
        got = _call1(fx.fx_sqrt_fast, x)
        bad = ~_same_bits(got, ref)
        assert not bad.any(), (seed, x[bad][:5], got[bad][:5], ref[bad][:5])
    z = _call1(fx.fx_sqrt_fast, np.array([0.0, -0.0]))
    assert not np.signbit(z[0]) and np.signbit(z[1]) and (z == 0.0).all()          # sqrt(+0) = +0 on the short path, sqrt(-0) = -0


def test_bare_core_equals_sqrt_from_its_lower_end_upwards_and_on_the_radii(fx):
    """gs_sqrt_core: no test, no special values.  [2^-767, +inf) is the range where the compiler's expansion scales by 2^0; the
    Box-Muller radii take it on [2^-32, 45.8], both ends of which are evaluated here through the header's logarithm."""
    rng = np.random.default_rng(11)
    ends = _radius_arguments(fx)
    assert 2.0 ** -32 <= ends[1] < 2.0 ** -31 and 45.0 < ends[0] < 45.8
    x = np.concatenate([_log_uniform(rng, 2.0 ** -32, 45.8, N), _log_uniform(rng, TINY, np.finfo(np.float64).max, N // 4),
                        _neighbours(_binade_ends()), [TINY, np.nextafter(TINY, 1.0), np.finfo(np.float64).max], ends,
                        _neighbours(np.arange(1.0, 7.0) ** 2)])
    ref = np.sqrt(x)
    for seed in (4, 5):
        fx.fx_seed(seed)
        got = _call1(fx.fx_sqrt_core, x)
        bad = ~_same_bits(got, ref)
        assert not bad.any(), (seed, x[bad][:5], got[bad][:5], ref[bad][:5])


def test_division_equals_true_division_where_nothing_needs_scaling(fx):
    """gs_div_fast's domain: a normal divisor, a normal quotient (or a = +0).  Operands log-uniform over 2^-250 .. 2^250 with either
    sign keep every intermediate normal."""
    rng = np.random.default_rng(12)
    sgn = lambda n: rng.choice([-1.0, 1.0], n)
    a = np.concatenate([_log_uniform(rng, 2.0 ** -250, 2.0 ** 250, N) * sgn(N), _neighbours(_binade_ends()), np.zeros(4)])
    b = np.concatenate([_log_uniform(rng, 2.0 ** -250, 2.0 ** 250, N) * sgn(N), np.resize([3.0, 7.0, 1.0, 2.0 ** 0.5, 10.0], 6 * 81),
                        [3.0, -3.0, 2.0 ** -250, 2.0 ** 250]])
    ref = a / b
    for seed in (6, 7):
        fx.fx_seed(seed)
        got = _div(fx, a, b)
        bad = ~_same_bits(got, ref)
        assert not bad.any(), (seed, a[bad][:5], b[bad][:5], got[bad][:5], ref[bad][:5])
    # a = +0 over a positive divisor is +0 like the division's.  a = -0 is outside the function's domain and its header says what comes
    # out: +0 (the remainder of a zero quotient is +0), where / gives -0 -- the reason f2_angle's f / e keeps the division.
    z = _div(fx, np.array([0.0, -0.0]), np.array([3.0, 3.0]))
    assert (z == 0.0).all() and not np.signbit(z).any()


def test_logarithms_division_on_its_own_domain_and_the_logarithm_whatever_the_estimate(fx):
    """gs_log01 divides f by 2 + f with f in [-0.30, 0.42], f = +0 or |f| >= 2^-53."""
    rng = np.random.default_rng(13)
    f = np.concatenate([_log_uniform(rng, 2.0 ** -53, 0.42, N // 2), -_log_uniform(rng, 2.0 ** -53, 0.30, N // 2),
                        [0.0, 2.0 ** -53, -2.0 ** -53, 2.0 ** -52, 0.42, -0.30, np.sqrt(2.0) - 1.0, np.sqrt(0.5) - 1.0]])
    fx.fx_seed(8)
    got = _div(fx, f, 2.0 + f)
    ref = f / (2.0 + f)
    bad = ~_same_bits(got, ref)
    assert not bad.any(), (f[bad][:5], got[bad][:5], ref[bad][:5])
    assert got[N] == 0.0 and not np.signbit(got[N])                                 # f = +0 (u = 1/2, u = 1): s = +0
    # the logarithm itself: the same bits from every estimate, and those of the build whose estimates are the true quotients
    u = np.concatenate([(rng.integers(0, 1 << 32, 200000).astype(np.float64) + 0.5) / 4294967296.0,
                        [0.5, 1.0 - 2.0 ** -33, 0.5 / 4294967296.0, 1.0, 0.70710678118654752, 0.7071067811865476]])
    plain = _call1(fx.plain.fm_log01, u)
    for seed in (9, 10):
        fx.fx_seed(seed)
        assert np.array_equal(_call1(fx.fx_log01, u).view(np.uint64), plain.view(np.uint64))
    k = 200000
    assert plain[k] == -0.6931471805599453 and plain[k + 3] == 0.0                  # ln(1/2) to the bit; ln 1 = +0
    assert abs(plain[k + 1] - np.log1p(-2.0 ** -33)) <= np.spacing(2.0 ** -33)       # the top of the uniforms' range: about -2^-33, not 0
    assert plain[k + 1] < 0.0


def test_uniform_of_a_word_is_the_same_as_one_fused_multiply_add(fx):
    rng = np.random.default_rng(14)
    r = np.concatenate([rng.integers(0, 1 << 32, 100000, dtype=np.uint64), [0, 1, (1 << 32) - 1, 1 << 31, (1 << 31) - 1]]).astype(np.uint32)
    a, b = np.empty(len(r)), np.empty(len(r))
    fx.fx_unit32(r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _p(a), _p(b), len(r))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a, (r.astype(np.float64) + 0.5) / 4294967296.0) and a.min() > 0.0 and a.max() < 1.0
