"""CPU: the NumPy restatements of the policy-action TD targets (include/gridstep.h "policy-action TD targets")
against torch on the CPU, and the host logic of ``DeviceLearner``'s ``q_target`` argument.

``policy_rows_np(exact=True)`` against a float64 torch restatement of the reference's ``_get_action_and_log_prob``
(algorithms/offline.py:114-136) fed the same eps, rtol 1e-10: both sides float64 on the same float32-rounded operands; the heads' own
exp, tanh and log lie within 4 ulp of the library's.  Compared where ``1 - |a| > 1e-5`` only -- section 23's finding: closer to
saturation ``log(1 - a^2 + 1e-6)`` magnifies an ulp of ``a`` beyond any fixed relative tolerance -- and the inputs are chosen so that
this holds everywhere (asserted).  ``q_next_noise_np`` against ``_philox4x32`` under both tags.  ``td_policy_np`` against a loop that
writes out offline.py:175-178 with the project's bootstrap option: the same float64 operations, equal bit for bit."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import DeviceLearner, pathwise_tanh_np
from grid_fed_rl_gym_amd.rollout import _philox4x32, policy_rows_np, q_next_noise_np, td_policy_np

torch = pytest.importorskip("torch")

ACT = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}
D, A = 7, 3


def _actor(hidden, activation, seed):
    torch.manual_seed(seed)
    dims = [D] + hidden + [2 * A]
    mods = []
    for l in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            mods.append(ACT[activation]())
    return torch.nn.Sequential(*mods)


def _reference_head(actor, state, eps):
    """offline.py:114-136 with ``normal.rsample()`` written as mean + std * eps (what rsample computes from its own eps)"""
    mean, log_std = torch.chunk(actor(state), 2, dim=-1)
    log_std = torch.clamp(log_std, -20, 2)
    std = torch.exp(log_std)
    if eps is None:
        return torch.tanh(mean), None
    normal = torch.distributions.Normal(mean, std)
    x_t = mean + std * eps
    action = torch.tanh(x_t)
    log_prob = normal.log_prob(x_t)
    log_prob = log_prob - torch.log(1 - action.pow(2) + 1e-6)
    return action, log_prob.sum(dim=-1)


@pytest.mark.parametrize("hidden,activation", [([16, 16], "relu"), ([10], "tanh"), ([12, 9, 5], "elu"), ([], "relu")])
@pytest.mark.parametrize("stochastic", [True, False])
def test_policy_rows_np_matches_the_reference_actor_in_float64(hidden, activation, stochastic):
    rng = np.random.default_rng(0)
    n = 40
    obs = rng.normal(50.0, 20.0, (n, D))
    mean, std = obs.mean(axis=0), obs.std(axis=0) + 1e-6
    actor = _actor(hidden, activation, 3)
    pol = P.MLPPolicy.from_sequential(actor, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    eps = rng.normal(size=(n, A)) if stochastic else None
    pre, a, lp = policy_rows_np(pol, obs, eps, exact=True)
    assert pre.shape == (n, 2 * A) and a.shape == (n, A) and lp.shape == (n,) and pre.dtype == np.float64
    assert (1.0 - np.abs(a) > 1e-5).all(), "the inputs keep every action away from saturation"
    obs_n = ((obs - mean) * (1.0 / std)).astype(np.float32).astype(np.float64)
    tower = actor.double()
    with torch.no_grad():      # the float32-rounded parameters the restatement uses
        for prm in tower.parameters():
            prm.copy_(prm.float().double())
        want_a, want_lp = _reference_head(tower, torch.from_numpy(obs_n), None if eps is None else torch.from_numpy(eps))
    assert np.allclose(a, want_a.numpy(), rtol=1e-10, atol=0.0)
    if stochastic:
        assert np.allclose(lp, want_lp.numpy(), rtol=1e-10, atol=0.0)
    else:
        assert np.array_equal(a, pathwise_tanh_np(pre[:, :A]))
        zero = policy_rows_np(pol, obs, np.zeros((n, A)), exact=True)
        assert np.array_equal(zero[1], a) and np.array_equal(zero[2], lp)
    # the float32 contract: float32 values, close to the exact ones; and the head on given pre-head values
    pre32, a32, lp32 = policy_rows_np(pol, obs, eps)
    assert pre32.dtype == np.float32 and np.allclose(pre32, pre, rtol=1e-4, atol=1e-5)
    again = policy_rows_np(pol, obs, eps, pre_head=pre32)
    assert np.array_equal(again[1], a32) and np.array_equal(again[2], lp32)


def _normals(words):
    u = (np.asarray(words, dtype=np.float64) + 0.5) * (1.0 / 4294967296.0)
    ra, rb = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
    ta, tb = 2.0 * math.pi * u[1], 2.0 * math.pi * u[3]
    return [ra * math.cos(ta), ra * math.sin(ta), rb * math.cos(tb), rb * math.sin(tb)]


@pytest.mark.parametrize("terminal,tag", [(False, 0x514E5854), (True, 0x514E5445)])
def test_q_next_noise_np_is_philox_under_the_transitions_index(terminal, tag):
    assert (_lib.Q_NEXT_ROLLOUT_TAG, _lib.Q_NEXT_TERMINAL_TAG) == (0x514E5854, 0x514E5445)
    assert tag.to_bytes(4, "big") == (b"QNTE" if terminal else b"QNXT")
    seed, draw, B, A5 = 0x123456789ABCDEF, 7, 5, 5
    tb = np.array([[3, 1], [0, 4], [36, 0], [2, 2]])
    index = tb[:, 0] * B + tb[:, 1]
    got = q_next_noise_np(seed, draw, index, A5, terminal=terminal)
    assert got.shape == (4, A5)
    u64 = lambda x: np.array([x], dtype=np.uint64)
    for j, i in enumerate(index):
        for k in range(A5):
            w = _philox4x32(u64(i), u64(k >> 2), u64(draw), u64(tag), seed & 0xFFFFFFFF, seed >> 32)
            want = _normals([int(x[0]) for x in w])[k & 3]
            assert math.isclose(got[j, k], want, rel_tol=1e-12, abs_tol=1e-15), (j, k)
    # another order of the same (t, b) entries gives the same rows; the two tags, a draw and a seed give other noise
    perm = np.array([2, 0, 3, 1])
    assert np.array_equal(q_next_noise_np(seed, draw, index[perm], A5, terminal=terminal), got[perm])
    assert not np.array_equal(q_next_noise_np(seed, draw, index, A5, terminal=not terminal), got)
    assert not np.array_equal(q_next_noise_np(seed, draw + 1, index, A5, terminal=terminal), got)
    assert not np.array_equal(q_next_noise_np(seed + 1, draw, index, A5, terminal=terminal), got)
    assert np.array_equal(q_next_noise_np(seed, draw, index, 3, terminal=terminal), got[:, :3])
    assert q_next_noise_np(seed, draw, np.zeros(0, dtype=np.int64), 3).shape == (0, 3)


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
@pytest.mark.parametrize("alpha", [0.0, 0.2])
def test_td_policy_np_is_the_reference_lines_with_the_bootstrap_option(mask, alpha):
    rng = np.random.default_rng(3)
    T, B = 9, 5
    rew, lp, qm = rng.normal(size=(T, B)), rng.normal(size=(T, B)), rng.normal(size=(T, B))
    term = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8), size=(T, B))
    idx = np.argwhere(term != 0).astype(np.int32)
    rng.shuffle(idx)
    tq, tlp = rng.normal(size=len(idx)), rng.normal(size=len(idx))
    gamma, shift, scale = 0.97, 0.25, 0.5
    got = td_policy_np(rew, lp, qm, term, tq, idx, gamma, alpha, mask, shift, scale, terminal_log_probs=tlp)
    where = {(int(t), int(b)): e for e, (t, b) in enumerate(idx)}
    for t in range(T):
        for b in range(B):
            rewards = (rew[t, b] - shift) * scale
            if term[t, b] == 0:
                target_q = qm[t, b] - alpha * lp[t, b]                 # offline.py:177
                want = rewards + gamma * target_q                      # offline.py:178 with (1 - terminals) = 1
            elif term[t, b] & mask:
                e = where[(t, b)]
                want = rewards + gamma * (tq[e] - alpha * tlp[e])      # the same expression on the terminal observation
            else:
                want = rewards + gamma * 0.0                           # (1 - terminals) = 0
            assert got[t, b] == want, (t, b)
    # the terminal entries' values given as such; another order of the list
    values = tq - alpha * tlp
    assert np.array_equal(td_policy_np(rew, lp, qm, term, values, idx, gamma, alpha, mask, shift, scale), got)
    perm = rng.permutation(len(idx))
    assert np.array_equal(td_policy_np(rew, lp, qm, term, values[perm], idx[perm], gamma, alpha, mask, shift, scale), got)
    if mask == 0:
        terminals = (term != 0).astype(np.float64)
        target_q = qm - alpha * lp
        assert np.array_equal(got, (rew - shift) * scale + gamma * ((1 - terminals) * target_q))
        assert np.array_equal(td_policy_np(rew, lp, qm, term, [], np.zeros((0, 2)), gamma, alpha, 0, shift, scale), got)


def test_every_value_error_of_the_restatements():
    pol = P.MLPPolicy([np.zeros((2 * A, D))], [np.zeros(2 * A)], head="gaussian_tanh", compute="float32")
    plain = P.MLPPolicy([np.zeros((A, D))], [np.zeros(A)], head="tanh", compute="float32")
    obs = np.zeros((4, D))
    for call in (lambda: policy_rows_np(plain, obs, None), lambda: policy_rows_np(pol, np.zeros((4, D + 1)), None),
                 lambda: policy_rows_np(pol, np.zeros(D), None), lambda: policy_rows_np(pol, obs, np.zeros((4, A + 1))),
                 lambda: policy_rows_np(pol, obs, None, pre_head=np.zeros((4, A)))):
        with pytest.raises(ValueError):
            call()
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=True), dict(seed=1.5), dict(draw=-1), dict(draw=1 << 32), dict(draw=0.5), dict(A=0),
               dict(index=np.array([-1])), dict(index=np.array([1 << 32])), dict(index=np.zeros((2, 2), dtype=np.int64)), dict(index=np.array([0.5]))):
        args = dict(dict(seed=0, draw=0, index=np.arange(3), A=A), **kw)
        with pytest.raises(ValueError):
            q_next_noise_np(**args)
    z = np.zeros((3, 2))
    good = dict(rewards=z, next_log_probs=z, q_next_min=z, terminals=z.astype(np.uint8), terminal_q=[], terminal_index=np.zeros((0, 2)))
    assert td_policy_np(**good).shape == (3, 2)
    for kw in (dict(next_log_probs=np.zeros((3, 3))), dict(q_next_min=np.zeros((2, 2))), dict(terminals=np.zeros(6, dtype=np.uint8)),
               dict(rewards=np.zeros(6), next_log_probs=np.zeros(6), q_next_min=np.zeros(6), terminals=np.zeros(6, dtype=np.uint8)),
               dict(gamma=math.nan), dict(gamma=math.inf), dict(alpha=-0.1), dict(alpha=math.nan), dict(alpha=math.inf), dict(bootstrap_mask=4),
               dict(bootstrap_mask=-1), dict(bootstrap_mask=1, terminal_index=np.array([[0, 0]]), terminal_q=[])):
        with pytest.raises(ValueError):
            td_policy_np(**dict(good, **kw))
    for kw in (dict(alpha=-1.0), dict(alpha=math.nan), dict(alpha=math.inf), dict(stochastic=1), dict(seed=-1), dict(draw=1 << 32),
               dict(bootstrap=("ended",))):
        env = _Env()
        with pytest.raises(ValueError):
            P.evaluate_rollout_q_next(env, **kw)
        assert env.handle.calls == []
    with pytest.raises(ValueError):
        _lib.q_target_number("next")
    assert _lib.q_target_number("policy") == _lib.GS_Q_TARGET_POLICY == 1 and _lib.q_target_number("value") == _lib.GS_Q_TARGET_VALUE == 0


def test_the_config_struct_is_the_headers():
    import ctypes
    assert ctypes.sizeof(_lib.gs_q_next_config) == 64
    cfg = _lib.q_next_config(0.97, 0.2, 3, False, (1 << 64) - 1, 5, 0.5, 0.25)
    assert (cfg.struct_size, cfg.bootstrap_mask, cfg.stochastic, cfg.gamma, cfg.alpha, cfg.reward_shift, cfg.reward_scale, cfg.seed, cfg.draw) == \
        (64, 3, 0, 0.97, 0.2, 0.5, 0.25, (1 << 64) - 1, 5)
    assert ctypes.sizeof(_lib.gs_rollout_q_next) == 24 + 16 * 8 and ctypes.sizeof(_lib.gs_rollout_q_next_host) == 16 * 8


# ---- host logic: DeviceLearner's q_target on a recording handle (no device) ----
class _Handle:
    def __init__(self):
        self.calls = []

    def learner_create(self, net, cfg):
        self.calls.append(("create", net))

    def learner_set_loss(self, net, loss):
        self.calls.append(("loss", net, int(loss.kind)))

    def learner_set_signal(self, net, signal):
        self.calls.append(("signal", net, signal))

    def q_set_target_source(self, source):
        self.calls.append(("q_target", source))

    def rollout_evaluate_q_next(self, cfg):
        self.calls.append(("q_next", cfg))


class _Env:
    def __init__(self):
        self.handle = _Handle()


def test_device_learner_q_target():
    env = _Env()
    learner = DeviceLearner(env, nets=("policy", "q1", "q2"), policy_loss="pathwise", bc_coef=2.5, q_target="policy")
    assert env.handle.calls == [("create", 0), ("create", 5), ("create", 6), ("q_target", "policy")]
    assert learner.q_target == "policy"
    env.handle.calls.clear()
    learner.set_q_target("value")
    learner.set_q_target("policy")
    assert env.handle.calls == [("q_target", "value"), ("q_target", "policy")] and learner.q_target == "policy"
    with pytest.raises(ValueError):
        learner.set_q_target("next")
    # the default calls no new entry
    env = _Env()
    learner = DeviceLearner(env, nets=("value", "q1"))
    assert env.handle.calls == [("create", 1), ("create", 5)] and learner.q_target == "value"
    # a learner without a Q network cannot move the handle's target
    env = _Env()
    learner = DeviceLearner(env, nets=("policy",))
    env.handle.calls.clear()
    with pytest.raises(ValueError):
        learner.set_q_target("policy")
    assert env.handle.calls == []


@pytest.mark.parametrize("kw", [dict(nets=("policy", "value"), q_target="policy"), dict(nets=("q1",), q_target="next"),
                                dict(nets=("policy",), q_target="policy", policy_loss="pathwise")])
def test_device_learner_refuses_q_target_before_anything_is_created(kw):
    env = _Env()
    with pytest.raises(ValueError):
        DeviceLearner(env, **kw)
    assert env.handle.calls == []
