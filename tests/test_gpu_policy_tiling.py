"""GPU: the MLP policy kernels (gs_k_policy_mlp, gs_k_policy_mlp_f32) at the edges of their tiling and head -- every row of
tests/policy_cases.py (one 16-block of input, obs_dim a multiple of 16 / even / odd, the float32 panel loop, layers of 1 .. 16
column tiles, one and four layers, a narrow layer between two wide ones, batches around the 32-row tile, action_dim 1 and 12), the
stochastic head beyond its first noise quad, the log_std clamp, and float32 handles with different LDS footprints side by side.
tests/test_policy_cases_static.py holds the table to its coverage and its policies to their input conditions on the host.

One environment per (feeder, solver, B), reused by all of its rows through set_policy: after reset(seed=3) and two steps of random
actions the instances differ, and policy_actions() evaluates the installed policy there without stepping.

Bounds.  float64: 1e-9 absolute, the bound of tests/test_gpu_policy.py (its derivation covers 1511 terms as it covers 684: the dot
product rounds at about 1e-13).  float32: the rule of tests/test_gpu_policy_f32.py, |device - float64 evaluation of the rounded
operands| <= 4 E_ref, with E_ref from NumPy alone on the same policy over 1024 observations of the same feeder (16 random steps of
64 instances: at least 1024 action values even for action_dim 1, whatever the row's B).  Every row is evaluated three times: as
drawn, with the first layer's weights on the last observation column zeroed, and with the last hidden unit's outgoing weights
zeroed; NumPy says each of the two moves some action by at least 100 bars, and the device must move with it -- the last real
column and row of each padded tile are read.  Noise: zero last-layer weights and a float32-representable log_std bias make the
action tanh(exp(clip(log_std, -20, 2)) eps), held against the oracle's Philox at rtol 1e-13.

The draws are rebuilt by policy_cases.eps_of, whose sine and cosine are accurate relative to their own size: cos(2 pi u) as written
rounds the angle first and is up to 3e-12 off, relatively, next to a zero crossing (tests/test_policy_cases_static.py measures it).

Measured (MI355X).  float64: largest error over all rows and variants 8.8e-12.  float32: E_ref 7.4e-8 .. 1.1e-6, device error
0.05 .. 1.06 x E_ref over the rows (1.06: obs_dim 1511 into 17 units; the two-panel rows lie at 0.62 .. 1.06), 0.89 and 1.12 on the
stochastic rollouts.  tanh(std * eps) and the clamp: 4.6e-16 relative at most.  The large float32 handle returns the same bits
after the small one is installed: its launches are not refused although the attribute was lowered in between."""
import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd.rollout import rollout_device
from tests import policy_cases as C

pytestmark = pytest.mark.gpu

TOL_POLICY = 1e-9           # tests/test_gpu_policy.py
MOVES = 100.0               # tests/test_policy_cases_static.py
POOL_B, POOL_T = 64, 16     # the observations E_ref is taken over


def _environment(name, B):
    fs = C.feeder(name)
    env = P.BatchedGridEnvironment(fs, num_envs=B, **C.env_kw(fs, C.SOLVER[name]))
    assert (env.obs_dim, env.action_dim) == C.WIDTHS[name]
    return env


@pytest.fixture(scope="module")
def handles():
    """get(feeder, B) -> (environment, the observations [B, obs_dim] it stands at); every environment is built once"""
    cache = {}

    def get(name, B):
        if (name, B) not in cache:
            env = _environment(name, B)
            env.reset(seed=3)
            rollout_device(env, 2, seed=5, reset=False)
            obs = env.handle.rollout_download(want=("final_observation",))["final_observation"]
            assert len({o.tobytes() for o in obs}) == B
            cache[(name, B)] = (env, obs)
        return cache[(name, B)]

    yield get
    for env, _ in cache.values():
        env.close()


@pytest.fixture(scope="module")
def pool():
    """get(feeder) -> 1024 observations of that feeder (16 random steps of 64 instances), computed once and never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            env = _environment(name, POOL_B)
            env.reset(seed=21)
            rollout_device(env, POOL_T, seed=22, reset=False)
            obs = env.handle.rollout_download(want=("observations",))["observations"].reshape(POOL_T * POOL_B, env.obs_dim)
            env.close()
            obs.setflags(write=False)
            cache[name] = obs
        return cache[name]

    return get


def _bar(pol, pool_obs, eps=None):
    """the bound the policy's device actions are held to"""
    if pol.compute == "float64":
        return TOL_POLICY, None
    e = C.e_ref(pol, pool_obs, eps)
    assert e > 0.0 and pool_obs.shape[0] * pol.action_dim >= 1000
    return 4.0 * e, e


def _evaluate(env, pol, obs, pool_obs, what):
    """the device's actions under `pol` where the environment stands, held to the policy's bar instance by instance"""
    env.set_policy(pol)
    assert env.policy_compute == pol.compute
    got = env.policy_actions()
    assert got.shape == (env.num_envs, env.action_dim) and got.dtype == np.float64
    want = C.reference(pol, obs)
    bar, e = _bar(pol, pool_obs)
    err = np.max(np.abs(got - want), axis=1)
    if e is None:
        print(f"{what}: max |device action - forward_np| {err.max():.3e}")
    else:
        print(f"{what}: E_ref {e:.3e}  max |device action - exact| {err.max():.3e}  ratio {err.max() / e:.2f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bar), (what, int(np.argmax(err)), float(err.max()), bar)
    return got, want, bar


def _check_row(row, handles, pool):
    env, obs = handles(row.feeder, row.B)
    pool_obs = pool(row.feeder) if row.compute == "float32" else None
    got0, want0, bar0 = _evaluate(env, C.policy(row), obs, pool_obs, C.row_id(row))
    print(f"{C.row_id(row)}: fraction of actions in (-0.99, 0.99): {float(np.mean(np.abs(want0) < 0.99)):.2f}")
    for variant in C.VARIANTS[1:]:
        pol = C.policy(row, variant)
        if pol is None:             # (no hidden unit to take away: policy_cases.policy)
            continue
        got, want, bar = _evaluate(env, pol, obs, pool_obs, f"{C.row_id(row)} [{variant} zeroed]")
        moved = float(np.max(np.abs(want - want0)))
        assert moved >= MOVES * max(bar, bar0), (variant, moved, bar, bar0)            # NumPy: the column / the unit matters here
        assert np.max(np.abs((got - got0) - (want - want0))) <= bar + bar0, variant    # and the device moves with it
    env.set_policy(None)


@pytest.mark.parametrize("row", [r for r in C.TABLE if not (r.feeder == "chain3" and r.hidden == (64,))], ids=C.row_id)
def test_tiling_edges_against_numpy(row, handles, pool):
    _check_row(row, handles, pool)


@pytest.mark.parametrize("row", [r for r in C.TABLE if r.feeder == "chain3" and r.hidden == (64,)], ids=C.row_id)
def test_batch_edges_every_instance_matches(row, handles, pool):
    """B = 1, 31, 32, 33, 64, 65 around the 32-row tile: the row clamp min(row, B - 1) and the head's b >= B break; _evaluate
    holds every instance's action row to the bar and the result to exactly [B, A]"""
    assert row.B in C.BATCHES
    _check_row(row, handles, pool)


def _stochastic_rollout(env, T, seed):
    env.reset(seed=3)
    rollout_device(env, T, seed=seed, reset=False, policy=True)
    return env.handle.rollout_download(want=("observations", "actions"))


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("name", C.HEAD_FEEDERS)
def test_stochastic_head_beyond_the_first_noise_quad(name, compute):
    """action_dim 12 and 5: noise quads 0 .. 2, components 0 .. 3.  B = 64, T = 4: 1280 action values at action_dim 5"""
    B, T, seed = 64, 4, 0x1234567890ABCDEF
    env = _environment(name, B)
    A = env.action_dim
    pol = C.policy(C.Row(name, C.SOLVER[name], B, (256, 256), "relu", "gaussian_tanh", compute))
    env.set_policy(pol, stochastic=True)
    d = _stochastic_rollout(env, T, seed)
    eps = C.eps_of(seed, 0, T, B, A)
    bar, e = _bar(pol, d["observations"].reshape(T * B, -1), eps.reshape(T * B, A))
    err = float(np.max(np.abs(d["actions"] - C.reference(pol, d["observations"], eps))))
    print(f"stochastic {name} {compute}: max |device action - reference| {err:.3e}" + ("" if e is None else f"  E_ref {e:.3e}  ratio {err / e:.2f}"))
    assert err <= bar, (err, bar)
    noise = np.abs(d["actions"] - C.reference(pol, d["observations"]))
    assert np.all(noise.reshape(T * B, A).max(axis=0) > 1e-3)                          # the noise is there, on every action
    # gs_policy_mlp_eval draws what rollout step t draws
    env.reset(seed=3)
    assert np.array_equal(env.policy_actions(seed=seed, t=0), d["actions"][0])
    # the draw itself (rtol 1e-13, atol 0): mean exactly 0, log_std exactly its float32-representable bias
    log_std = np.linspace(-1.0, 0.0, A).astype(np.float32).astype(np.float64)
    only, held = C.head_only_policy(name, log_std, compute)
    assert np.array_equal(held, log_std) and len(set(held)) == A
    env.set_policy(only, stochastic=True)
    dn = _stochastic_rollout(env, T, seed)
    env.close()
    want = np.tanh(np.exp(held) * eps)
    print(f"noise only {name} {compute}: max relative error of tanh(std * eps) per action:", np.max(np.abs(dn["actions"] - want) / np.abs(want), axis=(0, 1)))
    assert np.allclose(dn["actions"], want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_log_std_clamp_at_both_bounds(compute):
    name, B, T, seed = C.HEAD_FEEDERS[0], 33, 2, 77
    env = _environment(name, B)
    A = env.action_dim
    pol, held = C.head_only_policy(name, C.CLAMP_LOG_STD, compute)
    assert np.any(held < -20.0) and np.any(held > 2.0)
    env.set_policy(pol, stochastic=True)
    d = _stochastic_rollout(env, T, seed)
    env.close()
    eps = C.eps_of(seed, 0, T, B, A)
    want = np.tanh(np.exp(np.clip(held, -20.0, 2.0)) * eps)
    print(f"clamp {compute}: max relative error per action:", np.max(np.abs(d["actions"] - want) / np.abs(want), axis=(0, 1)))
    assert np.allclose(d["actions"], want, rtol=1e-13, atol=0)
    unclamped = np.tanh(np.exp(held) * eps)
    for out in (held < -20.0, held > 2.0):                 # (the bound is there: without it the actions are others)
        assert not np.allclose(d["actions"][..., out], unclamped[..., out], rtol=1e-6, atol=0)


def test_float32_handles_with_different_lds_footprints_coexist(pool):
    """gs_k_policy_mlp_f32 takes 159 KB of dynamic LDS for obs_dim 1511 and 35 KB for obs_dim 16; the limit a launch is checked
    against is set per FUNCTION, i.e. shared by every handle of the process: installing the small policy after the large one must
    not take the large one's launches away.  A float64 policy on a third handle in between."""
    B = 33
    big, small, third = _environment("chain252", B), _environment("chain2", B), _environment("star8", B)
    p_big = C.policy(C.Row("chain252", "fbs", B, (256, 256), "relu", "tanh", "float32"))
    p_small = C.policy(C.Row("chain2", "fbs", B, (256, 256), "relu", "gaussian_tanh", "float32"))
    p_third = C.policy(C.Row("star8", "fbs", B, (256, 256), "elu", "gaussian_tanh", "float64"))
    obs = {}
    for env in (big, small, third):
        env.reset(seed=3)
        rollout_device(env, 2, seed=5, reset=False)
        obs[env] = env.handle.rollout_download(want=("final_observation",))["final_observation"]
    a_big, _, _ = _evaluate(big, p_big, obs[big], pool("chain252"), "large float32 policy")
    a_small, _, _ = _evaluate(small, p_small, obs[small], pool("chain2"), "small float32 policy, installed after it")
    a_third, _, _ = _evaluate(third, p_third, obs[third], None, "float64 policy on a third handle")
    for _ in range(2):
        assert np.array_equal(big.policy_actions(), a_big)
        assert np.array_equal(small.policy_actions(), a_small)
        assert np.array_equal(third.policy_actions(), a_third)
    # the rollout's launches as well as gs_policy_mlp_eval's, and a small policy installed once more in between
    small.set_policy(p_small)
    rollout_device(big, 2, reset=False, policy=True)
    assert np.array_equal(big.handle.rollout_download(want=("actions",))["actions"][0], a_big)
    assert np.array_equal(small.policy_actions(), a_small)
    # the other order: the large policy installed after the small one
    big.set_policy(p_big)
    rollout_device(small, 2, reset=False, policy=True)
    assert np.array_equal(small.handle.rollout_download(want=("actions",))["actions"][0], a_small)
    for env in (big, small, third):
        env.close()
