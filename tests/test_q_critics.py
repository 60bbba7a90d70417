"""CPU: the NumPy restatements of the state-action critics (include/gridstep.h "state-action critics") against
torch on the CPU, and the host logic of ``MLPQ`` and of ``DeviceLearner``'s new arguments.

``q_rollout_np(exact=True)`` against a float64 torch ``TwinCritic``-shaped forward on ``cat(obs_n, act)`` (the operands rounded to
float32 first, as the device rounds them): both sides float64, summation order the only difference, rtol 1e-10.  ``td_target_np``
against a loop that writes out algorithms/offline.py:505 with the project's bootstrap option: the same float64 operations, equal
bit for bit.  ``polyak_np`` against torch's ``tau * p + (1 - tau) * t`` in float32: equal bit for bit.  The Q gradient is
``value_grad_np`` on the concatenated input: against torch autograd at section 19's tolerances (rtol 1e-10, atol 1e-12 max|g|)."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import DeviceLearner, value_grad_np
from grid_fed_rl_gym_amd.rollout import polyak_np, q_combine_np, q_rollout_np, td_target_np

torch = pytest.importorskip("torch")

ACT = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}
D, A = 7, 3


def _tower(dims, activation, seed):
    torch.manual_seed(seed)
    mods = []
    for l in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            mods.append(ACT[activation]())
    return torch.nn.Sequential(*mods)


class TwinCritic(torch.nn.Module):
    """the shape of the reference's CQL critic: two Sequential towers q1, q2 over cat(state, action)"""

    def __init__(self, hidden, activation):
        super().__init__()
        self.q1 = _tower([D + A] + hidden + [1], activation, 1)
        self.q2 = _tower([D + A] + hidden + [1], activation, 2)

    def forward(self, state, action):
        x = torch.cat([state, action], dim=-1)
        return self.q1(x), self.q2(x)


def _data(seed=0, T=6, B=4):
    rng = np.random.default_rng(seed)
    obs = rng.normal(50.0, 20.0, (T, B, D))
    act = rng.uniform(-1.0, 1.0, (T, B, A))
    mean, std = obs.reshape(-1, D).mean(axis=0), obs.reshape(-1, D).std(axis=0) + 1e-6
    return obs, act, mean, std


@pytest.mark.parametrize("hidden,activation", [([16, 16], "relu"), ([10], "tanh"), ([12, 9, 5], "elu"), ([], "relu")])
def test_q_rollout_np_matches_a_float64_twin_critic(hidden, activation):
    obs, act, mean, std = _data()
    twin = TwinCritic(hidden, activation)
    q1, q2 = P.MLPQ.twins(twin, obs_mean=mean, obs_std=std)
    assert q1.obs_dim == D and q1.action_dim == A and q1.activation == (activation if hidden else "relu")
    obs_n = ((obs - mean) * (1.0 / std)).astype(np.float32).astype(np.float64)
    a32 = act.astype(np.float32).astype(np.float64)
    with torch.no_grad():
        w1, w2 = twin.double()(torch.from_numpy(obs_n), torch.from_numpy(a32))
    for q, want in ((q1, w1), (q2, w2)):
        got = q_rollout_np(q, obs, act, exact=True)
        assert got.shape == obs.shape[:2] and got.dtype == np.float64
        assert np.allclose(got, want.numpy()[..., 0], rtol=1e-10, atol=0.0)
        f32 = q_rollout_np(q, obs, act)
        assert np.allclose(f32, got, rtol=1e-4, atol=1e-5) and np.array_equal(f32, f32.astype(np.float32).astype(np.float64))
    assert np.array_equal(q1.input_f32(obs, act)[..., D:], act.astype(np.float32))


def test_a_tower_of_linear_layers_alone_takes_the_activation_by_name():
    """IQL's TwinCritic keeps ModuleLists of Linear layers and the activation beside them"""
    twin = TwinCritic([8, 8], "tanh")
    holder = type("Holder", (), {})()
    holder.q1 = [m for m in twin.q1 if hasattr(m, "weight")]
    holder.q2 = [m for m in twin.q2 if hasattr(m, "weight")]
    holder.activation = torch.nn.Tanh()
    obs, act, mean, std = _data(1)
    a, b = P.MLPQ.twins(holder, obs_dim=D), P.MLPQ.twins(twin, obs_dim=D)
    for x, y in zip(a, b):
        assert x.activation == "tanh" and np.array_equal(x.forward_np(obs, act), y.forward_np(obs, act))
    with pytest.raises(ValueError):
        P.MLPQ.from_sequential(twin.q1)                   # neither obs_dim nor a normalisation
    with pytest.raises(ValueError):
        P.MLPQ.from_sequential(twin.q1, obs_dim=D + A)    # no action column left
    with pytest.raises(ValueError):
        P.MLPQ.from_sequential(twin.q1, obs_dim=D, obs_mean=np.zeros(D + 1), obs_std=np.ones(D + 1))
    with pytest.raises(ValueError):
        P.MLPQ.from_sequential(_tower([D + A, 4, 2], "relu", 0), obs_dim=D)      # two outputs


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_td_target_np_is_the_reference_line_with_the_bootstrap_option(mask):
    rng = np.random.default_rng(3)
    T, B = 9, 5
    rew, values = rng.normal(size=(T, B)), rng.normal(size=(T + 1, B))
    term = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8), size=(T, B))
    idx = np.argwhere(term != 0).astype(np.int32)
    rng.shuffle(idx)
    tv = rng.normal(size=len(idx))
    gamma, shift, scale = 0.97, 0.25, 0.5
    got = td_target_np(rew, values, term, tv, idx, gamma, mask, shift, scale)
    where = {(int(t), int(b)): float(v) for (t, b), v in zip(idx, tv)}
    for t in range(T):
        for b in range(B):
            r = (rew[t, b] - shift) * scale
            if term[t, b] == 0:
                want = r + gamma * values[t + 1, b]      # offline.py:505 with (1 - terminal) = 1: reward + discount * next_v
            elif term[t, b] & mask:
                want = r + gamma * where[(t, b)]
            else:
                want = r + gamma * 0.0                   # (1 - terminal) = 0
            assert got[t, b] == want, (t, b)
    if mask == 0:
        assert np.array_equal(got, (rew - shift) * scale + gamma * np.where(term != 0, 0.0, values[1:]))


def test_q_combine_np():
    rng = np.random.default_rng(4)
    a, b, c, d, v = (rng.normal(size=(3, 4)) for _ in range(5))
    values = np.concatenate([v, rng.normal(size=(1, 4))])
    on, tg, adv = q_combine_np([a, b], [c, d], values)
    assert np.array_equal(on, np.minimum(a, b)) and np.array_equal(tg, np.minimum(c, d)) and np.array_equal(adv, np.minimum(a, b) - v)
    on, tg, adv = q_combine_np([None, b], [None, d], values)
    assert np.array_equal(on, b) and np.array_equal(tg, d) and np.array_equal(adv, b - v)


@pytest.mark.parametrize("tau", [0.005, 0.5, 1.0, 0.0, 0.3])
def test_polyak_np_is_torchs_soft_update_in_float32_bit_for_bit(tau):
    rng = np.random.default_rng(5)
    p, t = rng.normal(size=1000).astype(np.float32), rng.normal(size=1000).astype(np.float32)
    got = polyak_np(p, t, tau)
    want = (tau * torch.from_numpy(p) + (1.0 - tau) * torch.from_numpy(t)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if tau == 1.0:
        assert np.array_equal(got.view(np.uint32), p.view(np.uint32))
    if tau == 0.0:
        assert np.array_equal(got.view(np.uint32), t.view(np.uint32))
    assert np.array_equal(polyak_np(np.zeros(4, np.float32), np.zeros(4, np.float32), tau).view(np.uint32), np.zeros(4, np.uint32))      # padding stays +0


@pytest.mark.parametrize("tau", [-0.1, 1.5, math.nan, math.inf])
def test_polyak_np_refuses_what_the_abi_refuses(tau):
    with pytest.raises(ValueError):
        polyak_np(np.zeros(2), np.zeros(2), tau)


@pytest.mark.parametrize("activation", ["relu", "tanh", "elu"])
def test_the_q_gradient_is_value_grad_np_on_the_concatenated_input(activation):
    obs, act, mean, std = _data(6, T=8, B=5)
    twin = TwinCritic([16, 12], activation)
    q1, _ = P.MLPQ.twins(twin, obs_mean=mean, obs_std=std)
    n = obs.shape[0] * obs.shape[1]
    sa = q1.input_f32(obs, act).reshape(n, D + A)
    y = np.random.default_rng(7).normal(size=n).astype(np.float32)
    layers = list(zip(q1.weights, q1.biases))
    ex = value_grad_np(layers, sa, y, exact=True, activation=activation)
    # (the same float64 operands; the two matrix products differ in shape, hence at most in summation order)
    assert np.allclose(ex["values"], q_rollout_np(q1, obs, act, exact=True).reshape(n), rtol=1e-12, atol=1e-14)
    tower = twin.q1.double()
    with torch.no_grad():      # the float32-rounded parameters the restatement uses
        for prm in tower.parameters():
            prm.copy_(prm.float().double())
    out = tower(torch.from_numpy(sa.astype(np.float64)))[:, 0]
    loss = ((out - torch.from_numpy(y.astype(np.float64))) ** 2).mean()
    loss.backward()
    lin = [m for m in tower if hasattr(m, "weight")]
    assert math.isclose(ex["loss"], float(loss.detach()), rel_tol=1e-12)
    for (dW, db), m in zip(ex["grads"], lin):
        for got, want in ((dW, m.weight.grad.numpy()), (db, m.bias.grad.numpy())):
            scale = float(np.max(np.abs(want)))
            assert np.allclose(got, want, rtol=1e-10, atol=1e-12 * scale)


# ---- host logic: names, numbers and every ValueError of the new arguments (no device: the handle is a recorder) ----
class _Handle:
    def __init__(self):
        self.calls = []

    def learner_create(self, net, cfg):
        self.calls.append(("create", net))

    def learner_set_loss(self, net, loss):
        self.calls.append(("loss", net, int(loss.kind)))

    def learner_set_signal(self, net, signal):
        self.calls.append(("signal", net, signal))

    def q_target_update(self, tau):
        self.calls.append(("targets", tau))


class _Env:
    def __init__(self):
        self.handle = _Handle()


def test_names_and_numbers_of_the_q_learners():
    assert _lib.GS_LEARNER_Q == 5 and _lib.learner_net("q1") == 5 and _lib.learner_net("q2") == 6
    assert _lib._net_number("q2") == 6 and _lib._net_number(6) == 6 and _lib._net_number(3) == 3 and _lib._net_number("thermal") == 4
    for bad in (7, 9, -1, "q3"):
        with pytest.raises(ValueError):
            _lib.learner_net(bad)
        with pytest.raises(ValueError):
            _lib._net_number(bad)
    assert _lib.q_which("q2") == 1 and _lib.q_which(0) == 0
    for bad in (2, -1, "q0", True):
        with pytest.raises(ValueError):
            _lib.q_which(bad)
    assert _lib.SIGNALS == {"batch": 0, "q": 1}


def test_device_learner_arguments_for_an_iql_learner():
    env = _Env()
    learner = DeviceLearner(env, nets=("policy", "value", "q1", "q2"), policy_loss="awr", value_loss="expectile", advantage_source="q",
                            value_target="q")
    assert env.handle.calls == [("create", 0), ("loss", 0, _lib.GS_LOSS_AWR), ("signal", 0, "q"), ("create", 1), ("loss", 1, _lib.GS_LOSS_EXPECTILE),
                                ("signal", 1, "q"), ("create", 5), ("create", 6)]
    assert learner.advantage_source == "q" and learner.value_target == "q"
    env.handle.calls.clear()
    learner.update_targets()
    learner.update_targets(tau=1.0)
    assert env.handle.calls == [("targets", 0.005), ("targets", 1.0)]
    for tau in (-0.01, 1.01, math.nan, math.inf):
        with pytest.raises(ValueError):
            learner.update_targets(tau)
    with pytest.raises(ValueError):
        learner.set_signal("q1", "q")
    with pytest.raises(ValueError):
        learner.set_signal("policy", "returns")
    with pytest.raises(ValueError):
        learner.value("q1")
    # the defaults call neither new entry; the Q learners take their own loss
    env = _Env()
    DeviceLearner(env, nets=("value", "q1"), value_loss="expectile", q_loss="mse")
    assert env.handle.calls == [("create", 1), ("loss", 1, _lib.GS_LOSS_EXPECTILE), ("create", 5)]
    env = _Env()
    DeviceLearner(env, nets=("q2",), q_loss="expectile")
    assert env.handle.calls == [("create", 6), ("loss", 6, _lib.GS_LOSS_EXPECTILE)]


@pytest.mark.parametrize("kw", [dict(nets=("value", "q1"), advantage_source="q"), dict(nets=("policy", "q1"), value_target="q"),
                                dict(nets=("policy",), advantage_source="td"), dict(nets=("value",), value_target="returns"),
                                dict(nets=("q1",), q_loss="awr"), dict(nets=("q1", "q1")), dict(nets=("q3",))])
def test_device_learner_refuses_before_anything_is_created(kw):
    env = _Env()
    with pytest.raises(ValueError):
        DeviceLearner(env, **kw)
    assert env.handle.calls == []
