"""CPU: the NumPy restatement of the conservative critic step (include/gridstep.h "the conservative critic step")
against torch autograd on the CPU, its candidate actions against Philox, the overflow branch of its logsumexp, and the host logic of
``DeviceLearner``'s new arguments.

``cql_grad_np(exact=True)`` against float64 torch autograd of a literal restatement of the reference's ``CQL._update_critic`` and
``CQL._compute_cql_loss`` (algorithms/offline.py:181-196 and 205-228): ``F.mse_loss(Q(s, a), y)`` plus ``conservative_weight`` times
``logsumexp(cat([Q(s, random), Q(s, policy), Q(s, a)], dim=0), dim=0) - Q(s, a).mean()``, the logsumexp over the BATCH.  Both sides
float64 on the same float32-rounded operands, at section 19's tolerances (rtol 1e-10, atol 1e-12 max|g|)."""
import math

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import (CQL_EXP_FLOOR, DeviceLearner, _block_sum_np, cql_grad_np, cql_noise_np, cql_uniform_np, pathwise_noise_np,
                                         value_grad_np)
from grid_fed_rl_gym_amd.rollout import _philox4x32

torch = pytest.importorskip("torch")
F = torch.nn.functional

D, A = 7, 3
CW = 5.0
ACT = {"relu": torch.relu, "tanh": torch.tanh, "elu": F.elu}


def _layers(dims, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0.0, scale / math.sqrt(dims[l]), (dims[l + 1], dims[l])), rng.normal(0.0, 0.1, dims[l + 1])) for l in range(len(dims) - 1)]


def _data(seed, n):
    """observations, the three action blocks and the targets, all float32-representable (the device's inputs are float32)"""
    rng = np.random.default_rng(seed)
    f = lambda x: x.astype(np.float32).astype(np.float64)
    return (f(rng.normal(0.0, 1.0, (n, D))), f(np.tanh(rng.normal(0.0, 1.0, (n, A)))), f(rng.uniform(-1.0, 1.0, (n, A))),
            f(np.tanh(rng.normal(0.0, 1.0, (n, A)))), f(rng.normal(0.0, 1.0, n)))


def _tower(params, state, action, activation):
    """one tower of the reference's TwinCritic (offline.py:80-101): Linear layers over cat([state, action]), [n, 1]"""
    x = torch.cat([state, action], dim=-1)
    for l, (w, b) in enumerate(params):
        x = x @ w.T + b
        if l < len(params) - 1:
            x = ACT[activation](x)
    return x


def _torch_critic(towers, obs, data, random, policy, y, cw, activation):
    """the reference's critic loss over the given towers (one: a twin on its own; two: the reference's sum), float64 on the
    float32-rounded operands; returns (loss, [[(dW, db)] per tower], [q over the 3 n rows in the DEVICE's order data | random | policy])"""
    r32 = lambda x: torch.from_numpy(np.asarray(x).astype(np.float32).astype(np.float64))
    params = [[(r32(w).requires_grad_(True), r32(b).requires_grad_(True)) for w, b in layers] for layers in towers]
    states, actions, random_actions, policy_actions = r32(obs), r32(data), r32(random), r32(policy)
    target_q = r32(y)[:, None]
    q_loss, cql_loss, qs = 0.0, 0.0, []
    for p in params:
        current_q = _tower(p, states, actions, activation)                      # offline.py:181
        q_loss = q_loss + F.mse_loss(current_q, target_q)                       # :184-186
        random_q = _tower(p, states, random_actions, activation)                # :218
        policy_q = _tower(p, states, policy_actions, activation)                # :219
        cat_q = torch.cat([random_q, policy_q, current_q], dim=0)               # :222
        cql_loss = cql_loss + (torch.logsumexp(cat_q, dim=0) - current_q.mean()).squeeze()      # :225-228
        qs.append(torch.cat([current_q, random_q, policy_q], dim=0)[:, 0].detach().numpy())
    critic_loss = q_loss + cw * cql_loss                                        # :196
    critic_loss.backward()
    return float(critic_loss.detach()), [[(w.grad.numpy(), b.grad.numpy()) for w, b in p] for p in params], qs


def _close(got, want):
    return np.allclose(got, want, rtol=1e-10, atol=1e-12 * float(np.max(np.abs(want))))


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("name,hidden,activation", [("relu", [16, 12], "relu"), ("tanh", [16, 12], "tanh"), ("elu", [16, 12], "elu"), ("single", [], "relu")])
def test_exact_restatement_against_torch_autograd_of_the_reference_critic(name, hidden, activation, n):
    obs, data, random, policy, y = _data(3, n)
    towers = [_layers([D + A] + hidden + [1], 10 + w) for w in range(2)]
    ex = [cql_grad_np(t, obs, data, random, policy, y, CW, exact=True, activation=activation) for t in towers]
    total, both, _ = _torch_critic(towers, obs, data, random, policy, y, CW, activation)
    assert math.isclose(ex[0]["loss"] + ex[1]["loss"], total, rel_tol=1e-10)
    for w in range(2):
        loss, (grads,), (q,) = _torch_critic([towers[w]], obs, data, random, policy, y, CW, activation)
        assert math.isclose(ex[w]["loss"], loss, rel_tol=1e-10), (ex[w]["loss"], loss)
        assert _close(ex[w]["q"], q) and np.array_equal(ex[w]["values"], ex[w]["q"][:n])
        for (dW, db), (tW, tb), (sW, sb) in zip(ex[w]["grads"], grads, both[w]):
            assert _close(dW, tW) and _close(db, tb), float(np.max(np.abs(dW - tW)))
            # the per-twin separation: the summed two-twin loss has the one-twin gradient with respect to twin w
            assert _close(sW, tW) and _close(sb, tb)
        assert any(np.abs(g[0]).max() > 0.0 for g in grads)
        m, S, lse, qbar = ex[w]["scalars"]
        assert m == ex[w]["q"].max() and math.isclose(sum(ex[w]["weights"]), 1.0, rel_tol=1e-12) and ex[w]["penalty"] == lse - qbar
        assert math.isclose(ex[w]["loss"], ex[w]["value_loss"] + CW * ex[w]["penalty"], rel_tol=1e-15)
        assert set(value_grad_np(towers[w], np.concatenate([obs, data], axis=1), y, activation=activation)) <= set(ex[w])


def test_weight_zero_is_the_plain_critic_step_over_the_data_rows():
    obs, data, random, policy, y = _data(5, 33)
    tower = _layers([D + A, 16, 12, 1], 4)
    ex = cql_grad_np(tower, obs, data, random, policy, y, 0.0, exact=True)
    plain = value_grad_np(tower, np.concatenate([obs, data], axis=1), y, exact=True)
    assert math.isclose(ex["loss"], plain["loss"], rel_tol=1e-14) and np.array_equal(ex["loss_terms"], plain["loss_terms"])
    for (dW, db), (pW, pb) in zip(ex["grads"], plain["grads"]):
        assert _close(dW, pW) and _close(db, pb)


def test_the_float32_restatement_lies_near_the_exact_one_and_takes_the_devices_values():
    obs, data, random, policy, y = _data(7, 65)
    tower = _layers([D + A, 16, 12, 1], 6)
    ex = cql_grad_np(tower, obs, data, random, policy, y, CW, exact=True)
    lo = cql_grad_np(tower, obs, data, random, policy, y, CW)
    assert lo["grads"][0][0].dtype == np.float32 and np.max(np.abs(lo["q"] - ex["q"])) < 1e-5
    for (dW, db), (eW, eb) in zip(lo["grads"], ex["grads"]):
        assert np.allclose(dW, eW, rtol=0.0, atol=1e-5 * float(np.max(np.abs(eW))))
    assert math.isclose(lo["scalars"][1], math.fsum(np.exp(lo["q"] - lo["scalars"][0])), rel_tol=1e-13)
    # q= and scalars= replace the forward pass's values in the head alone
    q = lo["q"] + 0.25
    fed = cql_grad_np(tower, obs, data, random, policy, y, CW, q=q, scalars=(lo["scalars"][0] + 0.25, lo["scalars"][1]))
    assert np.array_equal(fed["q"], q) and np.array_equal(fed["weights"], lo["weights"])
    assert np.array_equal(fed["loss_terms"], (q[:65] - y) * (q[:65] - y))


def test_the_statistics_order_of_one_workgroup():
    rng = np.random.default_rng(0)
    for size in (1, 63, 1024, 1026, 3000):
        x = rng.normal(0.0, 1.0, size)
        assert math.isclose(_block_sum_np(x), math.fsum(x), rel_tol=0.0, abs_tol=1e-12)
    x = np.zeros(2048)
    x[5], x[1029], x[6] = 1.0, 2.0 ** -53, 2.0 ** -53              # (thread 5 adds entry 1029 to entry 5 first, and loses it; then thread 6's)
    assert _block_sum_np(x) == 1.0 and math.fsum(x) == 1.0 + 2.0 ** -52


@pytest.mark.parametrize("A_", [1, 3, 5, 8])
def test_uniform_actions_are_philox_words_strictly_inside_the_interval(A_):
    seed, draw, n = 0x5EED0123456789, 7, 37
    u = cql_uniform_np(seed, draw, n, A_)
    assert u.shape == (n, A_) and u.dtype == np.float64 and np.all(u > -1.0) and np.all(u < 1.0)
    for i in (0, 5, n - 1):
        for k in range(A_):
            c = lambda x: np.array([x], dtype=np.uint64)
            words = _philox4x32(c(i), c(k >> 2), c(draw), c(_lib.CQL_UNIFORM_TAG), seed & 0xFFFFFFFF, seed >> 32)
            word = int(words[k & 3][0])
            want = (word + 0.5) / 2147483648.0 - 1.0              # (exact in float64)
            assert u[i, k] == want and u[i, k] == float((2 * word + 1) - 2 ** 32) / 2.0 ** 32
    assert not np.array_equal(u, cql_uniform_np(seed, draw + 1, n, A_)) and not np.array_equal(u, cql_uniform_np(seed + 1, draw, n, A_))
    assert abs(float(cql_uniform_np(seed, draw, 4096, A_).mean())) < 0.05
    # the extreme words stay inside, in float64
    assert (0 + 0.5) / 2147483648.0 - 1.0 > -1.0 and (0xFFFFFFFF + 0.5) / 2147483648.0 - 1.0 < 1.0
    with pytest.raises(ValueError):
        cql_uniform_np(seed, draw, n, 0)


def test_the_policy_candidates_noise_has_a_tag_of_its_own():
    assert (_lib.CQL_NOISE_TAG, _lib.CQL_UNIFORM_TAG, _lib.PATHWISE_NOISE_TAG) == (0x43514C4E, 0x43514C55, 0x50574E4F)
    a, b = cql_noise_np(11, 2, 33, 3), pathwise_noise_np(11, 2, 33, 3)
    assert a.shape == b.shape and not np.any(a == b)
    assert np.array_equal(a, pathwise_noise_np(11, 2, 33, 3, tag=_lib.CQL_NOISE_TAG)) and abs(float(cql_noise_np(11, 2, 4096, 3).mean())) < 0.05


def test_the_overflow_branch_of_the_logsumexp():
    n = 33
    obs, data, random, policy, y = _data(9, n)
    tower = _layers([D + A, 16, 12, 1], 8)
    tower[-1] = (tower[-1][0] * 2000.0, tower[-1][1])
    for exact in (True, False):
        r = cql_grad_np(tower, obs, data, random, policy, y, CW, exact=exact)
        q = r["q"]
        assert q.max() - q.min() > 1400.0
        assert all(np.all(np.isfinite(g)) for pair in r["grads"] for g in pair) and np.isfinite(r["loss"]) and np.all(np.isfinite(r["weights"]))
        below = q - q.max() < CQL_EXP_FLOOR
        assert below.sum() > 0 and (~below).sum() > 1 and np.all(r["weights"][below] == 0.0) and np.all(r["weights"][~below] > 0.0)
        lse = r["scalars"][2]
        assert math.isclose(lse, float(np.logaddexp.reduce(q)), rel_tol=1e-12)
        # the candidate rows that were dropped have exactly zero gradient at the head: only the data rows' regression reaches them
        assert math.isclose(float(r["weights"].sum()), 1.0, rel_tol=1e-12)


def test_every_value_error_of_the_restatement():
    obs, data, random, policy, y = _data(1, 5)
    tower = _layers([D + A, 8, 1], 2)
    for cw in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            cql_grad_np(tower, obs, data, random, policy, y, cw)
    with pytest.raises(ValueError):
        cql_grad_np(tower, obs, data[:4], random, policy, y, CW)
    with pytest.raises(ValueError):
        cql_grad_np(tower, obs, data, random[:, 0], policy, y, CW)
    with pytest.raises(ValueError):
        cql_grad_np(_layers([D + A, 8, 2], 2), obs, data, random, policy, y, CW)
    with pytest.raises(ValueError):
        cql_grad_np(tower, obs[:, :5], data, random, policy, y, CW)


# ---- host logic of DeviceLearner's new arguments (no device: the handle is a recorder) ----
class _Handle:
    def __init__(self):
        self.calls, self.steps = [], {}

    def learner_create(self, net, cfg):
        self.calls.append(("create", net))

    def learner_set_loss(self, net, loss):
        self.calls.append(("loss", net, int(loss.kind)))

    def learner_set_signal(self, net, signal):
        self.calls.append(("signal", net, signal))

    def q_set_target_source(self, source):
        self.calls.append(("target", source))

    def learner_info(self, net):
        return dict(step=self.steps.get(net, 0))

    def learner_step(self, net, batch, n, stream=None):
        self.calls.append(("step", net, n))
        self.steps[net] = self.steps.get(net, 0) + 1

    def learner_step_conservative(self, net, batch, n, cfg, stream=None):
        self.calls.append(("conservative", net, n, cfg.conservative_weight, cfg.stochastic, cfg.seed, cfg.draw, cfg.struct_size))
        self.steps[net] = self.steps.get(net, 0) + 1

    def learner_conservative_view(self, stream=None):
        self.calls.append(("view",))
        return {}


class _Env:
    def __init__(self):
        self.handle = _Handle()


class _Obs:
    shape = (33, D)


BATCH = dict(observations=_Obs())


def test_the_default_learner_calls_no_new_entry():
    env = _Env()
    learner = DeviceLearner(env, nets=("policy", "q1", "q2"))
    learner.step(BATCH)
    assert env.handle.calls == [("create", 0), ("create", 5), ("create", 6), ("step", 0, 33), ("step", 5, 33), ("step", 6, 33)]
    env = _Env()
    DeviceLearner(env, nets=("q1",), conservative_weight=0.0, conservative_seed=4).step(BATCH)
    assert env.handle.calls == [("create", 5), ("step", 5, 33)]


def test_device_learner_arguments_for_a_conservative_critic():
    cfg = _lib.conservative_config()
    assert (cfg.struct_size, cfg.conservative_weight, cfg.stochastic) == (32, 5.0, 1) and _lib.conservative_config(stochastic=False).stochastic == 0
    assert _lib.CQL_MAX_N == (1 << 24) // 3
    env = _Env()
    learner = DeviceLearner(env, nets=("q1", "policy", "q2"), q_target="policy", conservative_weight=5.0, conservative_seed=11)
    assert env.handle.calls == [("create", 5), ("create", 0), ("create", 6), ("target", "policy")]
    env.handle.calls.clear()
    learner.step(BATCH)
    learner.step(BATCH)
    # the new entry at the twins' positions in `nets`; draw = that twin's steps taken: both twins of a step share it
    assert env.handle.calls == [("conservative", 5, 33, 5.0, 1, 11, 0, 32), ("step", 0, 33), ("conservative", 6, 33, 5.0, 1, 11, 0, 32),
                                ("conservative", 5, 33, 5.0, 1, 11, 1, 32), ("step", 0, 33), ("conservative", 6, 33, 5.0, 1, 11, 1, 32)]
    env.handle.calls.clear()
    learner.step_conservative(BATCH, "q2", conservative_weight=0.0, stochastic=False, draw=9)
    learner.step_conservative(BATCH, 5, seed=3)
    assert env.handle.calls == [("conservative", 6, 33, 0.0, 0, 11, 9, 32), ("conservative", 5, 33, 5.0, 1, 3, 2, 32)]
    learner.conservative_views()
    assert env.handle.calls[-1] == ("view",)
    # explicit use on a learner whose conservative_weight is 0
    env = _Env()
    plain = DeviceLearner(env, nets=("q1", "value"))
    env.handle.calls.clear()
    plain.step_conservative(BATCH, "q1", conservative_weight=2.0)
    plain.step(BATCH)
    assert env.handle.calls == [("conservative", 5, 33, 2.0, 1, 0, 0, 32), ("step", 5, 33), ("step", 1, 33)]
    for kw in (dict(conservative_weight=-1.0), dict(conservative_weight=math.nan), dict(conservative_weight=math.inf), dict(stochastic=2), dict(seed=-1),
               dict(seed=2 ** 64), dict(seed=1.5), dict(draw=-1), dict(draw=2 ** 32), dict(draw=True)):
        with pytest.raises(ValueError):
            plain.step_conservative(BATCH, "q1", **kw)
    with pytest.raises(ValueError):
        plain.step_conservative(BATCH, "value")
    with pytest.raises(ValueError):
        plain.step_conservative(BATCH, "q2")                      # (not one of this learner's networks)
    with pytest.raises(ValueError):
        DeviceLearner(_Env(), nets=("value",)).conservative_views()


@pytest.mark.parametrize("kw", [dict(nets=("policy", "value"), conservative_weight=5.0), dict(nets=("q1",), conservative_weight=5.0, q_loss="expectile"),
                                dict(nets=("q1",), conservative_weight=-0.1), dict(nets=("q1",), conservative_weight=math.nan),
                                dict(nets=("q1",), conservative_weight=math.inf), dict(nets=("q1",), conservative_weight=1.0, conservative_stochastic=1),
                                dict(nets=("q1",), conservative_weight=1.0, conservative_seed=-3), dict(nets=("q1",), conservative_weight=1.0, conservative_seed=2 ** 64),
                                dict(nets=("q1",), conservative_seed=1.5), dict(conservative_weight=-2.0)])
def test_device_learner_refuses_before_anything_is_created(kw):
    env = _Env()
    with pytest.raises(ValueError):
        DeviceLearner(env, **kw)
    assert env.handle.calls == []
