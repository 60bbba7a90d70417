"""The short exact square root and division (csrc/fastmath.h) on the device: the functions themselves through gs_debug_fastmath,
bit for bit against NumPy and the host build, and the step kernels that use them -- at the flat start, where every line carries
S = 0 exactly and the square root must return +0, and on stochastic steps against the oracle.

Element i of a gs_debug_fastmath call is thread i, and gs_sqrt_fast chooses between its short path and the general square root per
wavefront: the arrays below are laid out so that whole wavefronts of ordinary values (with +0 among them) take the short path and
the wavefronts holding the special values take the general one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from oracle import oracle_np as O
from tests.helpers import oracle_spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT, DIV, LOG01, SQRT_CORE = 0, 1, 2, 3
TINY = 2.0 ** -767
_dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def _device(op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.full_like(a, np.nan)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
    rc = _lib.load().gs_debug_fastmath(op, len(a), _p(a), _p(b) if b is not None else None, _p(out))
    assert rc == 0, _lib.load().gs_last_error(None)
    return out


def _same_bits(got, ref):
    return (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))


def _log_uniform(rng, lo, hi, n):
    e = rng.uniform(np.log2(lo), np.log2(hi), n)
    k = np.floor(e)
    return np.clip(np.ldexp(np.exp2(e - k), k.astype(np.int64)), lo, hi)


def _neighbours(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)])


def _binade_ends():
    k = np.arange(-40, 41)
    return np.concatenate([np.ldexp(1.0, k), np.nextafter(np.ldexp(1.0, k + 1), 0.0)])


@pytest.fixture(scope="module")
def host_log01(tmp_path_factory):
    out = tmp_path_factory.mktemp("fastmath_gpu") / "libfastmath_host.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-I", os.path.join(ROOT, "grid_fed_rl_gym_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "fastmath_host.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.fm_log01.argtypes = [_dp, _dp, ctypes.c_long]

    def f(u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        r = np.empty_like(u)
        lib.fm_log01(_p(u), _p(r), len(u))
        return r
    return f


def test_square_root_on_the_device_equals_numpy_bit_for_bit(host_log01):
    rng = np.random.default_rng(20)
    ordinary = _log_uniform(rng, TINY, np.finfo(np.float64).max, 4096)                  # 64 wavefronts on the short path
    with_zeros = _log_uniform(rng, 1e-12, 1e3, 128)
    with_zeros[::5] = 0.0                                                               # two more, +0 among ordinary values
    squares = np.concatenate([np.arange(1.0, 40.0) ** 2, rng.integers(1, 1 << 26, 200).astype(np.float64) ** 2])
    radii = -2.0 * host_log01((np.array([0.0, 2.0 ** 32 - 1.0]) + 0.5) / 4294967296.0)
    ordinary_named = np.concatenate([_neighbours(squares), _neighbours(_binade_ends()), [TINY, np.nextafter(TINY, 1.0)], radii])
    ordinary_named = np.resize(ordinary_named, -(-len(ordinary_named) // 64) * 64)      # whole wavefronts: still the short path
    special = np.concatenate([[0.0, -0.0, 5e-324, 2.0 ** -1050, np.inf, np.nan, -1.0, np.nextafter(TINY, 0.0), np.finfo(np.float64).tiny],
                              _log_uniform(rng, 5e-324, TINY, 64), _log_uniform(rng, 1e-3, 1e3, 55)])
    x = np.concatenate([ordinary, with_zeros, ordinary_named, special])
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(x)
    got = _device(SQRT, x)
    bad = ~_same_bits(got, ref)
    assert not bad.any(), (np.flatnonzero(bad)[:8], x[bad][:5], got[bad][:5], ref[bad][:5])
    z = got[4096:4096 + 128][::5]
    assert (z == 0.0).all() and not np.signbit(z).any()
    # the bare core on the range the Box-Muller radii take it on
    xr = np.concatenate([_log_uniform(rng, 2.0 ** -32, 45.8, 4096), radii, [2.0 ** -32, 45.8]])
    bad = ~_same_bits(_device(SQRT_CORE, xr), np.sqrt(xr))
    assert not bad.any(), xr[bad][:5]


def test_division_and_logarithm_on_the_device_equal_numpy_and_the_host_build(host_log01):
    rng = np.random.default_rng(21)
    sgn = lambda n: rng.choice([-1.0, 1.0], n)
    f = np.concatenate([_log_uniform(rng, 2.0 ** -53, 0.42, 1024), -_log_uniform(rng, 2.0 ** -53, 0.30, 1024), [0.0, 2.0 ** -53, -2.0 ** -53, 0.42, -0.30]])
    ends = _neighbours(_binade_ends())
    a = np.concatenate([_log_uniform(rng, 2.0 ** -250, 2.0 ** 250, 4096) * sgn(4096), f, ends, [0.0, 0.0]])
    b = np.concatenate([_log_uniform(rng, 2.0 ** -250, 2.0 ** 250, 4096) * sgn(4096), 2.0 + f, np.resize([3.0, 7.0, 10.0], len(ends)), [3.0, 2.0 ** -250]])
    got, ref = _device(DIV, a, b), a / b
    bad = ~_same_bits(got, ref)
    assert not bad.any(), (a[bad][:5], b[bad][:5], got[bad][:5], ref[bad][:5])
    assert not np.signbit(got[-2:]).any() and not np.signbit(got[4096 + 2048])          # +0 / b = +0 (f = +0: u = 1/2, u = 1)
    u = np.concatenate([(rng.integers(0, 1 << 32, 4096).astype(np.float64) + 0.5) / 4294967296.0,
                        [0.5, 1.0 - 2.0 ** -33, 0.5 / 4294967296.0, 1.0, 0.70710678118654752, 0.7071067811865476]])
    got, ref = _device(LOG01, u), host_log01(u)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), u[got != ref][:5]


SHAPES = [(lambda: P.ieee13_like(), 20), (lambda: P.ieee123_like(), 130)]      # B = 20: no multiple of 16; B = 130: nine workgroups, the last one ragged


@pytest.mark.parametrize("maker,B", SHAPES)
def test_flat_start_gives_exact_zeros_and_set_points(maker, B):
    """tolerance = 1e3: every instance stops at the flat start, where V_i = V_j on every line: S = 0 exactly, |S| = sqrt(+0)."""
    fs = maker()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, tolerance=1e3)
    env.reset(seed=np.arange(B, dtype=np.uint64) + 11)
    rng = np.random.default_rng(22)
    for _ in range(2):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (B, fs.action_dim)))
        n, m = fs.n, fs.m
        vm, va = obs[:, 0:2 * n:2], obs[:, 1:2 * n:2]
        flow, loading = obs[:, 2 * n:2 * n + 2 * m:2], obs[:, 2 * n + 1:2 * n + 2 * m:2]
        ratio = env.handle.debug_read_rows("LOAD")                                       # |S| / rating, row by row
        print(fs.n, B, "max |S|/rating", np.abs(ratio).max(), "max loading", np.abs(loading).max(), "max angle", np.abs(va).max(),
              "|V| range", vm.min(), vm.max(), "iterations", info["iterations"].min(), info["iterations"].max())
        assert np.isfinite(ratio).all() and np.isfinite(loading).all()
        assert (ratio == 0.0).all() and not np.signbit(ratio).any()
        assert (loading == 0.0).all() and (flow == 0.0).all()
        assert ((vm == np.asarray(fs.v_set)[None, :]) | (vm == 1.0)).all()
        assert (va == 0.0).all()
    env.close()


@pytest.mark.parametrize("maker,B,picks", [(SHAPES[0][0], 20, range(20)), (SHAPES[1][0], 130, (0, 17, 127, 129))])
def test_six_stochastic_steps_against_the_oracle(maker, B, picks):
    """Default solver tolerance, stochastic loads and weather: every load draw's logarithm, division and radius, the weather's, and the
    epilogue's |S| and |V| go through the short functions.  Observations against the oracle at the bar of tests/test_gpu_env.py."""
    fs = maker()
    T = 6
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True)
    seeds = np.arange(B, dtype=np.uint64) + 50
    env.reset(seed=seeds)
    actions = np.random.default_rng(23).uniform(-1, 1, (T, B, fs.action_dim))
    spec = oracle_spec(fs, stochastic_loads=True, weather_variation=True, power_base=fs.base_power_va, solver="fbs", tolerance=1e-6,
                       max_iterations=50, jacobian_mode="exact", zero_z="open")
    states = {b: O.env_reset(spec, seed=int(seeds[b]), instance=b)[1] for b in picks}
    worst = 0.0
    for t in range(T):
        obs, rew, term, trunc, info = env.step(actions[t])
        for b in picks:
            o, r, te, tr, inf = O.env_step(spec, states[b], actions[t, b])
            err = float(np.max(np.abs(obs[b] - o) / np.maximum(1.0, np.abs(o))))
            worst = max(worst, err)
            print(fs.n, "step", t, "instance", b, "max rel obs error", err, "iterations", int(info["iterations"][b]), int(inf["iterations"]))
            assert err < 1e-8, (t, b, err)
            assert abs(rew[b] - r) <= 1e-7 * max(1.0, abs(r))
        assert info["power_flow_converged"].all()
    env.close()
