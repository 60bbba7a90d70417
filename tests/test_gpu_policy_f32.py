"""GPU: the float32 compute path of the MLP policy (GS_COMPUTE_F32, gs_k_policy_mlp_f32) inside closed-loop rollouts.

Policies, normalisation and feeders are built as in tests/test_gpu_policy.py: weights N(0, 1 / fan_in), the normalisation from
a short random rollout with std = 1 on the columns that do not vary, so at least half of all actions lie in (-0.99, 0.99).

Bound.  E_ref is the largest absolute difference, on the test's own policy and the rollout's own observations, between two NumPy
evaluations: the float32 forward_np and the float64 evaluation of the same float32-rounded operands (exact=True).  It is a
property of float32 on that data, never computed from the device.  The device is held to |action - exact| <= 4 E_ref: it sums in
another order than NumPy (rounding errors of random sign grow with the square root of the chain) and uses its own float32 tanh /
expm1 in the hidden layers.  The 13-bus feeder's obs_dim is 71, so every 13-bus case is also the odd-obs_dim case; B = 37 and 200
are not multiples of the 32-row tile.  Measured (MI355X): E_ref 2.6e-7 .. 1.1e-6 over the cases, device error 0.85 .. 1.68 x E_ref.
Noise: as in test_gpu_policy.py, zero last-layer weights and a float32-representable log_std bias make the action tanh(std * eps),
held against the oracle's Philox at rtol 1e-13."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import rollout_device
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
TOL_F64 = 1e-9         # tests/test_gpu_policy.py's bound on the float64 kernel
WANT = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")


def _kw(fs, solver="fbs", episode_length=5):
    return dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                max_iterations=100 if solver == "fbs" else 50, power_base=fs.base_power_va, episode_length=episode_length)


def _normalisation(env):
    obs = P.collect_random_data(env, 4, seed=11)["observations"]
    mean, std = obs.mean(axis=0), obs.std(axis=0)
    constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
    return mean, np.where(constant, 1.0, std + 1e-6)


def _policies(env, head="gaussian_tanh", activation="relu", hidden=(256, 256), seed=0):
    """the same network twice: compute="float32" and compute="float64" """
    rng = np.random.default_rng(seed)
    dims = [env.obs_dim, *hidden, 2 * env.action_dim if head == "gaussian_tanh" else env.action_dim]
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    mean, std = _normalisation(env)
    return (P.MLPPolicy(ws, bs, activation=activation, head=head, obs_mean=mean, obs_std=std, compute="float32"),
            P.MLPPolicy(ws, bs, activation=activation, head=head, obs_mean=mean, obs_std=std))


def _eps(seed, first_instance, T, B, A):
    """eps[t, b, a] as tests/test_gpu_policy.py rebuilds it from the oracle's Philox (tag 'PNOI')"""
    out = np.empty((T, B, A))
    for t in range(T):
        for b in range(B):
            for q in range((A + 3) // 4):
                r = O.philox4x32(((first_instance + b) & 0xFFFFFFFF, t, q, 0x504E4F49), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
                u = [(x + 0.5) * (1.0 / 4294967296.0) for x in r]
                ra, rb = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
                z = (ra * math.cos(2.0 * math.pi * u[1]), ra * math.sin(2.0 * math.pi * u[1]),
                     rb * math.cos(2.0 * math.pi * u[3]), rb * math.sin(2.0 * math.pi * u[3]))
                for k in range(4):
                    if 4 * q + k < A:
                        out[t, b, 4 * q + k] = z[k]
    return out


def _rollout(env, T, seed=3, policy_seed=0):
    env.reset(seed=seed)
    rollout_device(env, T, seed=policy_seed, reset=False, policy=True)
    return env.handle.rollout_download(want=WANT)


def _assert_unsaturated(actions):
    frac = float(np.mean(np.abs(actions) < 0.99))
    print("fraction of actions in (-0.99, 0.99):", frac)
    assert frac >= 0.5, frac


def _e_ref(pol, obs, eps=None):
    e = float(np.max(np.abs(pol.forward_np(obs, eps, compute="float32") - pol.forward_np(obs, eps, compute="float32", exact=True))))
    assert e > 0.0
    return e


def _assert_actions(pol, obs, actions, eps=None, what=""):
    """|device - float64 evaluation of the rounded operands| <= 4 E_ref, E_ref from NumPy on these observations"""
    e_ref = _e_ref(pol, obs, eps)
    err = float(np.max(np.abs(actions - pol.forward_np(obs, eps, compute="float32", exact=True))))
    print(f"{what}E_ref {e_ref:.3e}  max |device action - exact| {err:.3e}  ratio {err / e_ref:.2f}")
    assert err <= 4.0 * e_ref, (err, e_ref)
    return e_ref


def _fresh_rows(d):
    tt, bb = np.nonzero(d["terminals"][:-1])
    assert d["n_terminal"] > 0 and len(tt) > 0
    fresh, terminal = d["observations"][tt + 1, bb], d["next_observations"][tt, bb]
    assert not np.any(np.all(fresh == terminal, axis=1))
    return tt, bb, fresh, terminal


def _assert_fresh_rows(pol, d, e_ref):
    """the rows the policy saw right after an in-place reset are the fresh observations, not the terminal ones"""
    tt, bb, fresh, terminal = _fresh_rows(d)
    assert np.max(np.abs(d["actions"][tt + 1, bb] - pol.forward_np(fresh, compute="float32", exact=True))) <= 4.0 * e_ref
    assert np.max(np.abs(d["actions"][tt + 1, bb] - pol.forward_np(terminal, compute="float32", exact=True))) > 1e-6


def _assert_environment_unchanged(fs, B, T, d, episode_length=5, **extra):
    """a second handle on the GS_POLICY_UPLOADED path, fed exactly these actions, reproduces everything bit for bit"""
    ref = P.BatchedGridEnvironment(fs, num_envs=B, **extra, **_kw(fs, episode_length=episode_length))
    ref.reset(seed=3)
    rollout_device(ref, T, actions=d["actions"], reset=False)
    r = ref.handle.rollout_download(want=WANT)
    ref.close()
    assert r["n_terminal"] == d["n_terminal"]
    for k in WANT:
        assert np.array_equal(r[k], d[k]), k


@pytest.mark.parametrize("feeder,B,head,activation,hidden", [
    ("ieee13", 37, "gaussian_tanh", "relu", (256, 256)),
    ("ieee13", 37, "tanh", "elu", (256, 256, 256)),
    ("ieee13", 200, "tanh", "tanh", (100, 37)),
    ("ieee123", 200, "gaussian_tanh", "tanh", (256, 256)),
    ("ieee123", 200, "tanh", "relu", (100, 37)),
    ("ieee123", 37, "gaussian_tanh", "elu", (256, 256, 256)),
])
def test_float32_policy_accuracy_against_float64_policy_and_environment_unchanged(feeder, B, head, activation, hidden):
    fs = FEEDERS[feeder]()
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    if feeder == "ieee13":
        assert env.obs_dim % 2 == 1            # (the odd-obs_dim case)
    p32, p64 = _policies(env, head, activation, hidden, seed=B)
    assert env.policy_compute is None
    env.set_policy(p32)
    assert env.policy_compute == "float32"
    obs0, _ = env.reset(seed=3)
    a0 = env.policy_actions()
    T = 12
    d = _rollout(env, T)
    assert np.array_equal(d["observations"][0], obs0) and np.array_equal(d["actions"][0], a0)
    e_ref = _assert_actions(p32, d["observations"], d["actions"], what=f"{feeder} B={B} {head} {activation} {hidden}: ")
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(p32, d, e_ref)
    # where the environment stands afterwards: gs_policy_mlp_eval acts on the final observation
    a_final = env.policy_actions()
    assert np.max(np.abs(a_final - p32.forward_np(d["final_observation"], compute="float32", exact=True))) <= 4.0 * e_ref
    # the float64 policy on the same observations (the handle stands at the final one): close, and not the same bits
    env.set_policy(p64)
    assert env.policy_compute == "float64"
    a64 = env.policy_actions()
    assert np.max(np.abs(a64 - p64.forward_np(d["final_observation"]))) <= TOL_F64
    diff = float(np.max(np.abs(a64 - a_final)))
    print("max |float64 policy - float32 policy|:", diff)
    assert diff <= 4.0 * e_ref + TOL_F64
    assert not np.array_equal(a64, a_final)
    env.close()
    _assert_environment_unchanged(fs, B, T, d)


def test_full_size_123_bus_8192_instances():
    fs = P.ieee123_like()
    B, T = 8192, 3
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, episode_length=2))
    assert env.handle.describe()["kernel"] == "fbs_flow2h"
    p32, p64 = _policies(env, seed=1)
    env.set_policy(p32)
    d = _rollout(env, T)
    e_ref = _assert_actions(p32, d["observations"], d["actions"], what="ieee123 B=8192: ")
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(p32, d, e_ref)
    a32 = env.policy_actions()
    env.set_policy(p64)
    a64 = env.policy_actions()
    env.close()
    assert np.max(np.abs(a64 - p64.forward_np(d["final_observation"]))) <= TOL_F64
    assert np.max(np.abs(a64 - a32)) <= 4.0 * e_ref + TOL_F64 and not np.array_equal(a64, a32)
    _assert_environment_unchanged(fs, B, T, d, episode_length=2)


@pytest.mark.parametrize("which", ["loads", "impedances"])
def test_float32_policy_on_per_instance_handles(which):
    fs = P.ieee13_like("epsilon")
    B, T = 37, 8
    extra = (dict(load_powers=P.randomized_load_powers(fs, B, seed=4, per_load=True)) if which == "loads"
             else dict(line_impedances=P.randomized_line_impedances(fs, B, rel=0.1, seed=2)))
    env = P.BatchedGridEnvironment(fs, num_envs=B, **extra, **_kw(fs))
    assert env.handle.describe()["per_instance_loads" if which == "loads" else "per_instance_z"] == 1
    p32, _ = _policies(env, seed=5)
    env.set_policy(p32)
    d = _rollout(env, T)
    env.close()
    e_ref = _assert_actions(p32, d["observations"], d["actions"], what=f"per-instance {which}: ")
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(p32, d, e_ref)
    _assert_environment_unchanged(fs, B, T, d, **extra)


def test_stochastic_head_draws_what_the_oracle_defines():
    fs = P.ieee13_like("epsilon")
    B, T, seed = 37, 7, 0x1234567890ABCDEF
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    A = env.action_dim
    p32, _ = _policies(env, seed=4)
    env.set_policy(p32, stochastic=True)
    d = _rollout(env, T, policy_seed=seed)
    eps = _eps(seed, 0, T, B, A)
    e_ref = _assert_actions(p32, d["observations"], d["actions"], eps, what="stochastic: ")
    _assert_unsaturated(d["actions"])
    assert d["n_terminal"] > 0
    assert np.max(np.abs(d["actions"] - p32.forward_np(d["observations"]))) > 1e-3              # (the noise is there at all)
    # gs_policy_mlp_eval draws what rollout step t draws
    env.reset(seed=3)
    assert np.array_equal(env.policy_actions(seed=seed, t=0), d["actions"][0])
    assert np.max(np.abs(env.policy_actions(seed=seed, t=5) - p32.forward_np(d["observations"][0], eps[5], compute="float32", exact=True))) <= 4.0 * e_ref
    again = _rollout(env, T, policy_seed=seed)
    for k in WANT:
        assert np.array_equal(again[k], d[k]), k
    other = _rollout(env, T, policy_seed=seed + 1)
    assert not np.array_equal(other["actions"], d["actions"])
    # the draw itself (rtol 1e-13, atol 0): mean exactly 0, log_std exactly its float32-representable bias
    ws = [p32.weight0.copy()] + [w.copy() for w in p32.weights[1:]]
    bs = [p32.bias0.copy()] + [b.copy() for b in p32.biases[1:]]
    ws[-1][:] = 0.0
    bs[-1][:A] = 0.0
    bs[-1][A:] = np.linspace(-1.0, 0.0, A).astype(np.float32).astype(np.float64)
    assert A == 1 or len(set(bs[-1][A:])) == A
    noise = P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=p32.obs_mean, obs_std=p32.obs_std, compute="float32")
    env.set_policy(noise, stochastic=True)
    dn = _rollout(env, T, policy_seed=seed)
    want = np.tanh(np.exp(bs[-1][A:]) * eps)
    print("max relative error of tanh(std * eps):", float(np.max(np.abs(dn["actions"] - want) / np.abs(want))))
    assert np.allclose(dn["actions"], want, rtol=1e-13, atol=0)
    # ... and the float64 kernel draws the same numbers from the same seed
    n64 = P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=p32.obs_mean, obs_std=p32.obs_std)
    env.set_policy(n64, stochastic=True)
    d64 = _rollout(env, T, policy_seed=seed)
    assert np.allclose(d64["actions"], want, rtol=1e-13, atol=0)
    env.close()


def test_state_rules_refusals_and_switching_precision():
    fs = P.ieee13_like("epsilon")
    B, T = 16, 4
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    lib, h = _lib.load(), env.handle
    p32, p64 = _policies(env, seed=2)
    env.set_policy(p32)
    obs, _ = env.reset(seed=1)                          # reset keeps the policy
    a32 = env.policy_actions()
    e_ref = _assert_actions(p32, obs, a32, what="state rules: ")
    state = env.get_state()
    env.step(np.zeros((B, env.action_dim)))
    env.set_state(state)                                # and so does set_state
    assert np.array_equal(env.policy_actions(), a32)
    ref32 = _rollout(env, T, seed=1)
    long32 = _rollout(env, 8, seed=1)                   # 8 steps: in-place resets happen, the policy goes on acting
    assert long32["n_terminal"] > 0
    _assert_actions(p32, long32["observations"], long32["actions"], what="across in-place resets: ")
    # refusals leave the installed float32 policy acting unchanged
    env.reset(seed=1)
    p, keep = p32.to_struct()
    for opts_kw, match in ((dict(compute="float32", struct_size=8), r"struct_size"), (dict(compute=7), r"unknown compute"),
                           (dict(compute="float64", obs_shift=p32.obs_mean, obs_scale=1.0 / p32.obs_std), r"GS_COMPUTE_F32"),
                           (dict(compute="float32", obs_shift=p32.obs_mean, obs_scale=np.full(env.obs_dim, np.nan)), r"obs_scale\[0\]")):
        o, keep_o = _lib.policy_opts(**opts_kw)
        with pytest.raises(P.PowerFlowError, match=r"-1.*" + match):
            h.set_policy(p, o)
    huge = P.MLPPolicy([np.full((env.action_dim, env.obs_dim), 1e39)], [np.zeros(env.action_dim)], head="tanh", compute="float32")
    with pytest.raises(P.PowerFlowError, match=r"-1.*not finite in float32"):
        env.set_policy(huge)
    assert env.policy_compute == "float32"
    assert np.array_equal(env.policy_actions(), a32)
    got = _rollout(env, T, seed=1)
    for k in WANT:
        assert np.array_equal(got[k], ref32[k]), k
    # float64 -> float32 -> float64 on one handle: the float64 bits come back; a refusal leaves the float64 policy alone too
    env.set_policy(p64)
    env.reset(seed=1)
    a64 = env.policy_actions()
    assert np.max(np.abs(a64 - p64.forward_np(obs))) <= TOL_F64 and not np.array_equal(a64, a32)
    ref64 = _rollout(env, T, seed=1)
    env.reset(seed=1)
    with pytest.raises(P.PowerFlowError, match=r"-1.*not finite in float32"):
        env.set_policy(huge)
    assert env.policy_compute == "float64" and np.array_equal(env.policy_actions(), a64)
    env.set_policy(p32)
    assert np.array_equal(env.policy_actions(), a32)
    env.set_policy(p64)
    assert np.array_equal(env.policy_actions(), a64)
    got = _rollout(env, T, seed=1)
    for k in WANT:
        assert np.array_equal(got[k], ref64[k]), k
    # explicit float64 options without shift / scale are gs_policy_mlp_set: the same bits
    env.reset(seed=1)
    p, keep = p64.to_struct()
    o, keep_o = _lib.policy_opts("float64")
    h.set_policy(p, o)
    assert np.array_equal(env.policy_actions(), a64)
    # None removes the policy
    env.set_policy(p32)
    env.set_policy(None)
    assert env.policy_compute is None
    with pytest.raises(P.PowerFlowError, match=r"-5.*gs_policy_mlp_set"):
        h.rollout(T, "mlp")
    with pytest.raises(P.PowerFlowError, match=r"-5.*gs_policy_mlp_set"):
        env.policy_actions()
    env.close()


def test_collect_policy_data_takes_a_float32_policy():
    fs = P.ieee13_like("epsilon")
    B, T = 16, 6
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    p32, _ = _policies(env, seed=3)
    d = P.collect_policy_data(env, p32, T, seed=2)
    assert env.policy_compute == "float32"
    env.close()
    assert d["terminals"].any()
    _assert_actions(p32, d["observations"], d["actions"], what="collect_policy_data: ")
