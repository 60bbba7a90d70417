"""GPU: closed-loop rollouts -- the MLP policy evaluated on the device between two steps of gs_rollout (GS_POLICY_MLP).

The policy kernel against MLPPolicy.forward_np on every observation of a rollout (the rows right after an in-place reset
included), the environment bit for bit against the GS_POLICY_UPLOADED path fed the same actions, the stochastic head against
noise rebuilt from the oracle's Philox, and the state rules (the policy is not environment state; refusals change nothing).

Bounds.  Policy arithmetic: 1e-9 absolute -- a 684-term float64 dot product with O(1) terms rounds at about 1e-13, three
1-Lipschitz layers keep that below 1e-11, and 1e-9 leaves two orders for the device's exp / tanh.  Noise: the bar
tests/test_stochastic.py holds the device's normal draws to (rtol = 1e-13, atol = 0 on a quantity linear in the draw,
test_stochastic.py:175), on a policy whose mean is exactly 0 and whose log_std is exactly its bias (zero last-layer weights), so
that the action is tanh(std * eps) and nothing but the draw, one exp and one tanh enters.
Weights are N(0, 1 / fan_in); the observation normalisation comes from a short random rollout, so pre-activations are O(1) and
at least half of all actions lie in (-0.99, 0.99): agreement cannot come from a saturated tanh.  Columns that do not vary at
all (the static load powers) get std = 1 instead of GridDataset's 0 + 1e-6: with 1e-6 their folded weights are 1e6 times the
others and a 1e5-watt entry cancels against the folded bias to an absolute 1e-5 in ANY summation order -- a property of that
normalisation, not of the kernel."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import rollout_device
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
TOL_POLICY = 1e-9
WANT = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")


def _kw(fs, solver="fbs", episode_length=5):
    return dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                max_iterations=100 if solver == "fbs" else 50, power_base=fs.base_power_va, episode_length=episode_length)


def _normalisation(env):
    obs = P.collect_random_data(env, 4, seed=11)["observations"]
    mean, std = obs.mean(axis=0), obs.std(axis=0)
    constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
    return mean, np.where(constant, 1.0, std + 1e-6)


def _policy(env, head="gaussian_tanh", activation="relu", hidden=(256, 256), seed=0):
    rng = np.random.default_rng(seed)
    dims = [env.obs_dim, *hidden, 2 * env.action_dim if head == "gaussian_tanh" else env.action_dim]
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    mean, std = _normalisation(env)
    return P.MLPPolicy(ws, bs, activation=activation, head=head, obs_mean=mean, obs_std=std)


def _eps(seed, first_instance, T, B, A):
    """eps[t, b, a]: component a & 3 of the four normals of one Philox call keyed by seed, counter (global instance, t, a // 4,
    'PNOI'): Box-Muller cosine and sine on words (0, 1) and (2, 3), u = (r + 1/2) 2^-32 -- the recipe of oracle_np.rng_normal_quad"""
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
    """reset(seed), then T steps under the installed policy; the downloaded arrays"""
    env.reset(seed=seed)
    rollout_device(env, T, seed=policy_seed, reset=False, policy=True)
    return env.handle.rollout_download(want=WANT)


def _assert_unsaturated(actions):
    frac = float(np.mean(np.abs(actions) < 0.99))
    print("fraction of actions in (-0.99, 0.99):", frac)
    assert frac >= 0.5, frac


def _assert_actions(pol, d, eps=None, tol=TOL_POLICY):
    want = pol.forward_np(d["observations"], eps)
    err = float(np.max(np.abs(d["actions"] - want)))
    print("max |device action - forward_np|:", err)
    assert err <= tol, err


def _assert_fresh_rows(pol, d):
    """the rows the policy saw right after an in-place reset are the fresh observations, not the terminal ones"""
    T = d["terminals"].shape[0]
    tt, bb = np.nonzero(d["terminals"][:-1])
    assert d["n_terminal"] > 0 and len(tt) > 0
    fresh, terminal = d["observations"][tt + 1, bb], d["next_observations"][tt, bb]
    assert not np.any(np.all(fresh == terminal, axis=1))
    assert np.max(np.abs(d["actions"][tt + 1, bb] - pol.forward_np(fresh))) <= TOL_POLICY
    assert np.max(np.abs(d["actions"][tt + 1, bb] - pol.forward_np(terminal))) > 1e-6       # (it did not act on the terminal rows)
    assert T > 1


@pytest.mark.parametrize("feeder,B,head,activation,hidden", [
    ("ieee13", 37, "gaussian_tanh", "relu", (256, 256)),
    ("ieee13", 37, "tanh", "elu", (256, 256, 256)),
    ("ieee123", 200, "gaussian_tanh", "tanh", (256, 256)),
    ("ieee123", 200, "tanh", "relu", (100, 37)),
])
def test_policy_arithmetic_against_numpy_and_environment_unchanged(feeder, B, head, activation, hidden):
    fs = FEEDERS[feeder]()
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    pol = _policy(env, head, activation, hidden, seed=B)
    env.set_policy(pol)
    obs0, _ = env.reset(seed=3)
    a0 = env.policy_actions()
    assert np.max(np.abs(a0 - pol.forward_np(obs0))) <= TOL_POLICY
    T = 12
    d = _rollout(env, T)
    assert np.array_equal(d["observations"][0], obs0) and np.array_equal(d["actions"][0], a0)
    _assert_actions(pol, d)
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(pol, d)
    # where the environment stands afterwards: gs_policy_mlp_eval acts on the final observation
    assert np.max(np.abs(env.policy_actions() - pol.forward_np(d["final_observation"]))) <= TOL_POLICY
    env.close()
    # the environment itself: a second handle on the untouched GS_POLICY_UPLOADED path, fed exactly these actions
    ref = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    ref.reset(seed=3)
    rollout_device(ref, T, actions=d["actions"], reset=False)
    r = ref.handle.rollout_download(want=WANT)
    ref.close()
    assert r["n_terminal"] == d["n_terminal"]
    for k in WANT:
        assert np.array_equal(r[k], d[k]), k


def test_full_size_123_bus_8192_instances():
    fs = P.ieee123_like()
    B, T = 8192, 3
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, episode_length=2))
    assert env.handle.describe()["kernel"] == "fbs_flow2h"
    pol = _policy(env, seed=1)
    env.set_policy(pol)
    d = _rollout(env, T)
    env.close()
    _assert_actions(pol, d)
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(pol, d)
    ref = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, episode_length=2))
    ref.reset(seed=3)
    rollout_device(ref, T, actions=d["actions"], reset=False)
    r = ref.handle.rollout_download(want=WANT)
    ref.close()
    for k in WANT:
        assert np.array_equal(r[k], d[k]), k


def test_stochastic_head_draws_what_the_oracle_defines():
    fs = P.ieee13_like("epsilon")
    B, T, seed = 37, 7, 0x1234567890ABCDEF
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    A = env.action_dim
    pol = _policy(env, seed=4)
    env.set_policy(pol, stochastic=True)
    d = _rollout(env, T, policy_seed=seed)
    eps = _eps(seed, 0, T, B, A)
    _assert_actions(pol, d, eps)
    _assert_unsaturated(d["actions"])
    assert d["n_terminal"] > 0
    assert np.max(np.abs(d["actions"] - pol.forward_np(d["observations"]))) > 1e-3            # (the noise is there at all)
    # gs_policy_mlp_eval draws what rollout step t draws
    env.reset(seed=3)
    assert np.array_equal(env.policy_actions(seed=seed, t=0), d["actions"][0])
    assert np.max(np.abs(env.policy_actions(seed=seed, t=5) - pol.forward_np(d["observations"][0], eps[5]))) <= TOL_POLICY
    # same seed: the same bits; another seed: other actions
    again = _rollout(env, T, policy_seed=seed)
    for k in WANT:
        assert np.array_equal(again[k], d[k]), k
    other = _rollout(env, T, policy_seed=seed + 1)
    assert not np.array_equal(other["actions"], d["actions"])
    # the draw itself at the bar of tests/test_stochastic.py:175 (rtol 1e-13, atol 0): mean exactly 0, log_std exactly its bias
    ws = [w.copy() for w in pol.weights]; bs = [b.copy() for b in pol.biases]
    ws[-1][:] = 0.0
    bs[-1][:A] = 0.0
    bs[-1][A:] = np.linspace(-1.0, 0.0, A)
    noise = P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh")
    env.set_policy(noise, stochastic=True)
    dn = _rollout(env, T, policy_seed=seed)
    want = np.tanh(np.exp(bs[-1][A:]) * eps)
    print("max relative error of tanh(std * eps):", float(np.max(np.abs(dn["actions"] - want) / np.abs(want))))
    assert np.allclose(dn["actions"], want, rtol=1e-13, atol=0)
    env.close()


def test_loopback_shards_draw_what_one_environment_draws():
    fs = P.ieee13_like("epsilon")
    B, T, seed = 24, 6, 77
    one = P.BatchedGridEnvironment(fs, num_envs=2 * B, **_kw(fs))
    pol = _policy(one, seed=9)
    one.set_policy(pol, stochastic=True)
    one.reset(seed=5)
    rollout_device(one, T, seed=seed, reset=False, policy=True)
    whole = one.handle.rollout_download(want=WANT)
    one.close()
    assert whole["n_terminal"] > 0
    pair = P.LoopbackShards(fs, 2 * B, 2, **_kw(fs))
    pair.reset(seed=5)
    for s in pair.shards:
        rollout_device(s.env, T, seed=seed, reset=False, policy=pol, stochastic=True)
        part = s.env.handle.rollout_download(want=WANT)
        for k in ("observations", "actions", "rewards", "next_observations", "terminals"):
            assert np.array_equal(part[k], whole[k][:, s.start:s.stop]), (k, s.rank)
        assert np.array_equal(part["final_observation"], whole["final_observation"][s.start:s.stop])
    pair.close()


def test_state_rules_and_refusals():
    fs = P.ieee13_like("epsilon")
    B, T = 16, 4
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    lib, h = _lib.load(), env.handle
    env.reset(seed=1)
    # no policy: GS_E_STATE from the rollout and from the evaluation
    with pytest.raises(P.PowerFlowError, match=r"-5.*gs_policy_mlp_set"):
        h.rollout(T, "mlp")
    with pytest.raises(P.PowerFlowError, match=r"-5.*gs_policy_mlp_set"):
        env.policy_actions()
    pol = _policy(env, seed=2)
    env.set_policy(pol)
    obs, _ = env.reset(seed=1)                          # reset keeps the policy
    assert np.max(np.abs(env.policy_actions() - pol.forward_np(obs))) <= TOL_POLICY
    state = env.get_state()
    env.step(np.zeros((B, env.action_dim)))
    env.set_state(state)                                # and so does set_state
    assert np.max(np.abs(env.policy_actions() - pol.forward_np(obs))) <= TOL_POLICY
    # a refused policy (wrong dims[0]; stochastic with the plain head) leaves the installed one and later steps alone
    ref = _rollout(env, T, seed=1)
    bad = P.MLPPolicy([np.zeros((env.action_dim, env.obs_dim + 1))], [np.zeros(env.action_dim)], head="tanh")
    env.reset(seed=1)
    with pytest.raises(P.PowerFlowError, match=r"-1.*dims\[0\]"):
        env.set_policy(bad)
    plain, keep = _lib.policy_struct([np.zeros((env.action_dim, env.obs_dim))], [np.zeros(env.action_dim)], head="tanh", stochastic=True)
    assert lib.gs_policy_mlp_set(h._h, plain) == _lib.GS_E_INVALID
    with pytest.raises(P.PowerFlowError, match=r"-1.*unknown policy"):
        h._check(lib.gs_rollout(h._h, T, 3, 0, None))
    rollout_device(env, T, reset=False, policy=True)
    got = h.rollout_download(want=WANT)
    for k in WANT:
        assert np.array_equal(got[k], ref[k]), k
    # NULL clears it
    env.set_policy(None)
    with pytest.raises(P.PowerFlowError, match=r"-5.*gs_policy_mlp_set"):
        h.rollout(T, "mlp")
    # ... and the random-action rollout behind all that is what a fresh handle collects
    fresh = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    a = P.collect_random_data(fresh, T, seed=6)
    b = P.collect_random_data(env, T, seed=6)
    fresh.close(); env.close()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_collect_policy_data_returns_the_reference_dictionary():
    fs = P.ieee13_like("epsilon")
    B, T = 16, 6
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    pol = _policy(env, seed=3)
    d = P.collect_policy_data(env, pol, T, seed=2)
    env.close()
    assert set(d) == {"observations", "actions", "rewards", "next_observations", "terminals"}
    assert d["observations"].shape == (T * B, env.obs_dim) and d["actions"].shape == (T * B, env.action_dim)
    assert d["terminals"].dtype == bool and d["terminals"].any()
    assert np.max(np.abs(d["actions"] - pol.forward_np(d["observations"]))) <= TOL_POLICY


@pytest.mark.parametrize("which", ["loads", "impedances"])
def test_policy_on_per_instance_handles(which):
    fs = P.ieee13_like("epsilon")
    B, T = 37, 8
    extra = (dict(load_powers=P.randomized_load_powers(fs, B, seed=4, per_load=True)) if which == "loads"
             else dict(line_impedances=P.randomized_line_impedances(fs, B, rel=0.1, seed=2)))
    env = P.BatchedGridEnvironment(fs, num_envs=B, **extra, **_kw(fs))
    assert env.handle.describe()["per_instance_loads" if which == "loads" else "per_instance_z"] == 1
    pol = _policy(env, seed=5)
    env.set_policy(pol)
    d = _rollout(env, T)
    env.close()
    _assert_actions(pol, d)
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(pol, d)
    ref = P.BatchedGridEnvironment(fs, num_envs=B, **extra, **_kw(fs))
    ref.reset(seed=3)
    rollout_device(ref, T, actions=d["actions"], reset=False)
    r = ref.handle.rollout_download(want=WANT)
    ref.close()
    for k in WANT:
        assert np.array_equal(r[k], d[k]), k


def test_policy_on_a_first_generation_member(monkeypatch):
    fs = P.ieee13_like("epsilon")
    B, T = 37, 8
    monkeypatch.setenv("GS_NO_FLOW2", "1")
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs))
    monkeypatch.delenv("GS_NO_FLOW2")
    assert "flow2" not in env.handle.describe()["kernel"]
    pol = _policy(env, seed=6)
    env.set_policy(pol)
    d = _rollout(env, T)
    env.close()
    _assert_actions(pol, d)
    _assert_unsaturated(d["actions"])
    _assert_fresh_rows(pol, d)
