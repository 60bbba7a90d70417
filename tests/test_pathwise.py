"""CPU: the NumPy restatement of the pathwise actor step (include/gridstep.h "the pathwise actor step") against
torch autograd on the CPU, its noise against the federation's recipe, and the host logic of ``DeviceLearner``'s new arguments.

``pathwise_grad_np(exact=True)`` against float64 torch autograd of the reference's ``CQL._update_actor`` form
(algorithms/offline.py:230-244: ``(alpha * log_prob - min(Q1, Q2)(s, pi(s))).mean()`` with ``pi(s)`` drawn by the reparameterisation
trick, offline.py:114-136, ``Normal(mean, std).log_prob(x) - log(1 - tanh(x)^2 + 1e-6)``), extended by ``bc_coef * |a - a_stored|^2``:
both sides float64 on the same float32-rounded operands, at section 19's tolerances (rtol 1e-10, atol 1e-12 max|g|).  The action
enters a twin rounded to float32, as the device rounds it; torch carries the gradient straight through that rounding."""
import math

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.federated import fed_noise_np
from grid_fed_rl_gym_amd.learner import DeviceLearner, pathwise_exp_np, pathwise_grad_np, pathwise_log_np, pathwise_noise_np, pathwise_tanh_np

torch = pytest.importorskip("torch")

D, A, N = 7, 3, 29
ACT = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}


def _layers(dims, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0.0, scale / math.sqrt(dims[l]), (dims[l + 1], dims[l])), rng.normal(0.0, 0.1, dims[l + 1])) for l in range(len(dims) - 1)]


def _data(seed=0, n=N):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (n, D)), rng.normal(0.0, 1.0, (n, A)), np.tanh(rng.normal(0.0, 1.0, (n, A)))


def _mlp(params, x, activation):
    for l, (w, b) in enumerate(params):
        x = x @ w.T + b
        if l < len(params) - 1:
            x = ACT[activation](x)
    return x


def _torch_actor(policy_layers, q_layers_list, obs_n, eps, alpha, bc_coef, stored, activation, q_activation):
    """the reference's actor loss in float64 on the float32-rounded operands; returns (loss, [(dW, db)] of the policy, q [twins, n])"""
    r32 = lambda x: torch.from_numpy(np.asarray(x).astype(np.float32).astype(np.float64))
    pol = [(r32(w).requires_grad_(True), r32(b).requires_grad_(True)) for w, b in policy_layers]
    qs = [[(r32(w), r32(b)) for w, b in layers] for layers in q_layers_list]
    obs, eps_t = r32(obs_n), torch.from_numpy(np.asarray(eps, dtype=np.float64))
    out = _mlp(pol, obs, activation)
    mean, log_std = out[:, :A], out[:, A:]
    std = torch.clamp(log_std, -20.0, 2.0).exp()
    x = mean + std * eps_t                                     # (rsample: the noise is a constant of the graph)
    a = torch.tanh(x)
    log_prob = (torch.distributions.Normal(mean, std).log_prob(x) - torch.log(1.0 - a.pow(2) + 1e-6)).sum(dim=-1)
    a_in = a + (a.detach().float().double() - a.detach())      # the value the twins see is float32(a); d/da = 1
    q = [_mlp(layers, torch.cat([obs, a_in], dim=-1), q_activation)[:, 0] for layers in qs]
    q_min = q[0] if len(q) == 1 else torch.min(q[0], q[1])
    loss = alpha * log_prob - q_min
    if bc_coef != 0.0:
        loss = loss + bc_coef * ((a - torch.from_numpy(np.asarray(stored, dtype=np.float64))) ** 2).sum(dim=-1)
    loss = loss.mean()
    loss.backward()
    return float(loss.detach()), [(w.grad.numpy(), b.grad.numpy()) for w, b in pol], torch.stack(q).detach().numpy()


def _compare(policy_layers, q_layers_list, obs, eps, alpha, bc_coef, stored, activation="relu", q_activation="relu"):
    ex = pathwise_grad_np(policy_layers, q_layers_list, obs, eps, alpha, bc_coef, stored_actions=stored, exact=True, activation=activation,
                          q_activation=q_activation)
    loss, grads, q = _torch_actor(policy_layers, q_layers_list, obs, eps, alpha, bc_coef, stored, activation, q_activation)
    assert math.isclose(ex["loss"], loss, rel_tol=1e-10), (ex["loss"], loss)
    assert np.allclose(ex["q"], q, rtol=1e-10, atol=1e-12 * float(np.max(np.abs(q))))
    for (dW, db), (tW, tb) in zip(ex["grads"], grads):
        for got, want in ((dW, tW), (db, tb)):
            assert np.allclose(got, want, rtol=1e-10, atol=1e-12 * float(np.max(np.abs(want)))), float(np.max(np.abs(got - want)))
    assert any(np.abs(g[0]).max() > 0.0 for g in grads)
    assert np.min(1.0 - np.abs(ex["actions"])) > 1e-5, "the comparison is made away from saturation (see the single-layer test)"
    return ex, grads


@pytest.mark.parametrize("activation", ["relu", "tanh", "elu"])
@pytest.mark.parametrize("stochastic", [True, False])
def test_exact_restatement_against_torch_autograd_of_the_reference_actor(activation, stochastic):
    obs, eps, stored = _data(1)
    eps = eps if stochastic else np.zeros_like(eps)
    pol = _layers([D, 16, 12, 2 * A], 1)
    qs = [_layers([D + A, 16, 12, 1], 10 + w) for w in range(2)]
    ex, _ = _compare(pol, qs, obs, eps, 0.2, 0.7, stored, activation, activation)
    assert 0 < ex["which"].sum() < N, "both twins are the smaller one somewhere"
    assert ex["surrogate"] == math.fsum(ex["q_min"]) / N and ex["entropy"] == -(math.fsum(ex["log_probs"]) / N)
    assert np.array_equal(ex["q_min"], np.where(ex["which"] == 0, ex["q"][0], ex["q"][1]))
    if not stochastic:
        f32 = pathwise_grad_np(pol, qs, obs, eps, 0.2, 0.7, stored_actions=stored, activation=activation, q_activation=activation)
        out = obs.astype(np.float32)
        for l, (w, b) in enumerate(pol):
            out = out @ w.astype(np.float32).T + b.astype(np.float32)
            if l < 2:
                out = {"relu": lambda v: np.maximum(v, np.float32(0)), "tanh": np.tanh,
                       "elu": lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, np.float32(0))))}[activation](out)
        assert np.array_equal(f32["actions"], pathwise_tanh_np(out[:, :A].astype(np.float64))), "the deterministic actor is tanh(mean)"


@pytest.mark.parametrize("alpha,bc_coef", [(0.0, 0.7), (0.2, 0.0), (0.0, 0.0)])
def test_alpha_zero_and_bc_zero(alpha, bc_coef):
    obs, eps, stored = _data(2)
    pol = _layers([D, 16, 2 * A], 2)
    qs = [_layers([D + A, 16, 1], 20 + w) for w in range(2)]
    ex, _ = _compare(pol, qs, obs, eps, alpha, bc_coef, stored if bc_coef else None)
    if bc_coef == 0.0:
        assert not ex["bc_terms"].any()
        assert np.array_equal(ex["loss_terms"], alpha * ex["log_probs"] - ex["q_min"])


def test_single_layer_policy_single_layer_q_and_one_twin_alone():
    obs, eps, stored = _data(3)
    # (a single layer on unit-variance inputs spreads log_std over +-3: std up to 20 saturates tanh to 1 - 1e-14, where 1 - a a is a
    # difference of two nearly equal numbers and one ulp of tanh -- NumPy's and torch's differ by that -- is 0.4 % of it.  The
    # comparison is made where the formula is well conditioned: weights and noise scaled so that 1 - |a| stays above 1e-5, which
    # _compare asserts.)
    eps = 0.2 * eps
    pol1, q1 = _layers([D, 2 * A], 3, scale=0.3), _layers([D + A, 1], 30)
    ex, _ = _compare(pol1, [q1, _layers([D + A, 1], 31)], obs, eps, 0.1, 0.5, stored)
    # a single-layer Q: dQ/da is the action columns of W0, whatever the sample
    w0 = q1[0][0].astype(np.float32)
    assert np.array_equal(ex["dq_da"][0], np.broadcast_to(w0[0, D:].astype(np.float64), (N, A)))
    f32 = pathwise_grad_np(pol1, [q1], obs, eps, 0.1, 0.5, stored_actions=stored)
    assert f32["dq_da"].dtype == np.float32 and np.array_equal(f32["dq_da"][0], np.broadcast_to(w0[0, D:], (N, A)))
    # one twin alone: the minimum is that twin
    pol = _layers([D, 16, 2 * A], 4)
    q = _layers([D + A, 16, 1], 32)
    one, _ = _compare(pol, [q], obs, eps, 0.1, 0.5, stored)
    assert not one["which"].any() and np.array_equal(one["q_min"], one["q"][0])


def test_a_log_std_outside_the_clamp_has_exactly_zero_gradient():
    """Above the clamp (std = e^2) the whole gradient is compared with torch; the noise is scaled by 0.2 so that tanh stays away from
    saturation (see the single-layer test).  Below it std = e^-20, and torch's own gradient with respect to the mean loses digits:
    Normal.log_prob's two paths, through x and through the mean, are each alpha eps / (n std) = 5e8 alpha eps / n and cancel to a
    rounding of that, 1e-10 and more.  So below the clamp the comparison runs at alpha = 0, where that term is absent, and at
    alpha > 0 the exact zeros are asserted on both sides."""
    obs, eps, stored = _data(4)
    eps = 0.2 * eps
    qs = [_layers([D + A, 16, 1], 40 + w) for w in range(2)]
    for push, alpha in ((30.0, 0.3), (-60.0, 0.0), (-60.0, 0.3)):
        pol = _layers([D, 16, 2 * A], 5)
        pol[-1][1][A + 1] = push       # beyond the clamp for every sample
        if push > 0.0 or alpha == 0.0:
            ex, grads = _compare(pol, qs, obs, eps, alpha, 0.2, stored)
        else:
            ex = pathwise_grad_np(pol, qs, obs, eps, alpha, 0.2, stored_actions=stored, exact=True)
            grads = _torch_actor(pol, qs, obs, eps, alpha, 0.2, stored, "relu", "relu")[1]
        assert ex["log_std_outside"][:, 1].all() and not ex["log_std_outside"][:, [0, 2]].all(axis=0).any()
        f32 = pathwise_grad_np(pol, qs, obs, eps, alpha, 0.2, stored_actions=stored)
        for g in (ex["grads"], grads, f32["grads"]):
            dW, db = g[-1]
            assert not dW[A + 1].any() and db[A + 1] == 0.0 and db[A] != 0.0 and db[A + 2] != 0.0, push


def test_which_replaces_the_choice_in_the_gradient_only():
    obs, eps, stored = _data(5)
    pol = _layers([D, 16, 2 * A], 6)
    qs = [_layers([D + A, 16, 1], 50 + w) for w in range(2)]
    ex = pathwise_grad_np(pol, qs, obs, eps, 0.1, 0.0, exact=True)
    flipped = pathwise_grad_np(pol, qs, obs, eps, 0.1, 0.0, exact=True, which=1 - ex["which"])
    assert np.array_equal(flipped["which"], ex["which"]), "`which` in the result is what the evaluation finds"
    assert not np.array_equal(flipped["q_min"], ex["q_min"]) and not np.array_equal(flipped["grads"][0][0], ex["grads"][0][0])
    same = pathwise_grad_np(pol, qs, obs, eps, 0.1, 0.0, exact=True, which=ex["which"])
    assert all(np.array_equal(a, b) for ga, gb in zip(same["grads"], ex["grads"]) for a, b in zip(ga, gb))


def test_the_float32_restatement_lies_near_the_exact_one():
    obs, eps, stored = _data(6)
    pol = _layers([D, 16, 12, 2 * A], 7)
    qs = [_layers([D + A, 16, 12, 1], 60 + w) for w in range(2)]
    ex = pathwise_grad_np(pol, qs, obs, eps, 0.2, 0.7, stored_actions=stored, exact=True)
    lo = pathwise_grad_np(pol, qs, obs, eps, 0.2, 0.7, stored_actions=stored, which=ex["which"])
    assert lo["dq_da"].dtype == np.float32 and all(g[0].dtype == np.float32 for g in lo["grads"])
    assert np.allclose(lo["q"], ex["q"], rtol=0.0, atol=1e-5 * float(np.max(np.abs(ex["q"]))))
    for (fW, fb), (eW, eb) in zip(lo["grads"], ex["grads"]):
        assert np.allclose(fW, eW, rtol=0.0, atol=1e-5 * float(np.max(np.abs(eW)))) and np.allclose(fb, eb, rtol=0.0, atol=1e-5 * float(np.max(np.abs(eb))))


@pytest.mark.parametrize("n,A_", [(1, 1), (5, 3), (7, 4), (3, 9)])
def test_noise_is_the_federations_recipe_under_the_actor_steps_counter(n, A_):
    seed, draw = 0x1234567890ABCDEF, 7
    got = pathwise_noise_np(seed, draw, n, A_)
    assert got.shape == (n, A_) and got.dtype == np.float64
    # fed_noise_np's counter is (quad, round, net, tag): sample i's quad q is the first word i with round = q and net = draw
    for i in range(n):
        for q in range((A_ + 3) // 4):
            want = fed_noise_np(seed, q, draw, 4 * (i + 1), tag=_lib.PATHWISE_NOISE_TAG)[4 * i:4 * i + 4]
            k = min(4, A_ - 4 * q)
            assert np.array_equal(got[i, 4 * q:4 * q + k], want[:k]), (i, q)
    assert _lib.PATHWISE_NOISE_TAG == int.from_bytes(b"PWNO", "big")
    assert not np.array_equal(got, pathwise_noise_np(seed, draw + 1, n, A_)) and not np.array_equal(got, pathwise_noise_np(seed + 1, draw, n, A_))
    big = pathwise_noise_np(3, 0, 4096, 4)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1.0) < 0.05


def _ulps(a, b):
    return int(np.max(np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))))


def test_the_heads_exp_tanh_and_log_against_numpys():
    """The heads' functions are sums of rounded float64 operations (so that device and host agree to the bit); against NumPy's own
    they must lie within 4 ulp over the ranges the heads use: exp on the clamp [-20, 2], tanh anywhere, log on [1e-6, 1 + 1e-6]."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-20.0, 2.0, 100000), [-20.0, 2.0, 0.0, -0.0, 1e-300]])
    assert _ulps(pathwise_exp_np(x), np.exp(x)) <= 4
    x = np.concatenate([rng.normal(0.0, 3.0, 100000), rng.uniform(-0.6, 0.6, 50000), 10.0 ** rng.uniform(-300, 0, 1000), [0.5, -0.5, 19.0, 45.0, -1e30]])
    assert _ulps(pathwise_tanh_np(x), np.tanh(x)) <= 4
    t = pathwise_tanh_np(np.array([0.0, -0.0, 1e30, -50.0, np.inf]))
    assert np.array_equal(t, [0.0, -0.0, 1.0, -1.0, 1.0]) and np.signbit(t[1]) and not np.signbit(t[0])
    assert np.all(np.abs(pathwise_tanh_np(x)) <= 1.0)
    v = np.concatenate([10.0 ** rng.uniform(-6.0, 0.0, 100000), (1.0 - 10.0 ** rng.uniform(-16.0, -1.0, 50000)) + 1e-6, [1e-6, 1.000001, 1.0, 0.5, 2.0]])
    assert _ulps(pathwise_log_np(v), np.log(v)) <= 4
    assert pathwise_log_np(np.array([1.0]))[0] == 0.0 and pathwise_exp_np(np.array([0.0]))[0] == 1.0


def test_every_value_error_of_the_restatements():
    obs, eps, stored = _data(7)
    pol = _layers([D, 8, 2 * A], 8)
    qs = [_layers([D + A, 8, 1], 70 + w) for w in range(2)]
    ok = dict(policy_layers=pol, q_layers_list=qs, obs_n=obs, eps=eps, alpha=0.1, bc_coef=0.5, stored_actions=stored)
    pathwise_grad_np(**ok)
    bad = [dict(alpha=-0.1), dict(alpha=math.nan), dict(alpha=math.inf), dict(bc_coef=-1.0), dict(bc_coef=math.nan), dict(bc_coef=math.inf),
           dict(eps=eps[:, :2]), dict(eps=eps[:-1]), dict(stored_actions=None), dict(stored_actions=stored[:, :2]), dict(q_layers_list=[]),
           dict(q_layers_list=qs + qs[:1]), dict(q_layers_list=[_layers([D + A + 1, 8, 1], 0)]), dict(q_layers_list=[_layers([D + A, 8, 2], 0)]),
           dict(obs_n=obs[:, :-1]), dict(which=np.full(N, 2)), dict(which=np.full(N, -1)), dict(activation="gelu"), dict(q_activation="gelu"),
           dict(policy_layers=_layers([D, 8, 2 * A + 1], 0))]
    for kw in bad:
        with pytest.raises(ValueError):
            pathwise_grad_np(**dict(ok, **kw))
    with pytest.raises(ValueError):
        pathwise_grad_np(pol, qs[:1], obs, eps, 0.1, 0.0, which=np.full(N, 1))      # one twin: only 0 can be named
    pathwise_grad_np(pol, qs, obs, eps, 0.1, 0.0)                                     # bc_coef = 0 needs no stored actions
    for args in ((0, 0, -1, 3), (0, 0, 4, 0), (0, 0, 4, -2)):
        with pytest.raises(ValueError):
            pathwise_noise_np(*args)
    assert pathwise_noise_np(0, 0, 0, 3).shape == (0, 3)


# ---- host logic of DeviceLearner's new arguments (no device: the handle is a recorder) ----
class _Handle:
    def __init__(self):
        self.calls, self.steps = [], 0

    def learner_create(self, net, cfg):
        self.calls.append(("create", net))

    def learner_set_loss(self, net, loss):
        self.calls.append(("loss", net, int(loss.kind)))

    def learner_get_loss(self, net):
        return dict(kind="default", temperature=0.0, weight_max=0.0, expectile=0.0)

    def learner_set_signal(self, net, signal):
        self.calls.append(("signal", net, signal))

    def learner_info(self, net):
        return dict(step=self.steps)

    def learner_step(self, net, batch, n, stream=None):
        self.calls.append(("step", net, n))

    def learner_step_pathwise(self, batch, n, cfg, stream=None):
        self.calls.append(("pathwise", n, cfg.alpha, cfg.bc_coef, cfg.stochastic, cfg.seed, cfg.draw, cfg.struct_size))
        self.steps += 1

    def learner_pathwise_view(self, stream=None):
        self.calls.append(("view",))
        return {}


class _Env:
    def __init__(self):
        self.handle = _Handle()


class _Obs:
    shape = (33, D)


def test_device_learner_arguments_for_a_pathwise_actor():
    assert _lib.pathwise_config().struct_size == 40 and _lib.pathwise_config(stochastic=False).stochastic == 0
    env = _Env()
    learner = DeviceLearner(env, nets=("value", "q1", "policy", "q2"), policy_loss="pathwise", alpha=0.2, bc_coef=2.5, pathwise_seed=11)
    # host state: the C loss kind is not involved, so the loss entry is never called
    assert env.handle.calls == [("create", 1), ("create", 5), ("create", 0), ("create", 6)]
    assert learner.loss("policy") == dict(kind="default", temperature=0.0, weight_max=0.0, expectile=0.0, name="pathwise", alpha=0.2, bc_coef=2.5,
                                          stochastic=True, seed=11)
    assert learner.loss("value")["name"] == "mse"
    env.handle.calls.clear()
    batch = dict(observations=_Obs())
    learner.step(batch)
    learner.step(batch)
    # the new entry at the policy's position in `nets`, draw = the policy's steps taken
    assert env.handle.calls == [("step", 1, 33), ("step", 5, 33), ("pathwise", 33, 0.2, 2.5, 1, 11, 0, 40), ("step", 6, 33),
                                ("step", 1, 33), ("step", 5, 33), ("pathwise", 33, 0.2, 2.5, 1, 11, 1, 40), ("step", 6, 33)]
    env.handle.calls.clear()
    learner.step_pathwise(batch, alpha=0.0, stochastic=False, draw=9)
    assert env.handle.calls == [("pathwise", 33, 0.0, 2.5, 0, 11, 9, 40)]
    learner.pathwise_views()
    assert env.handle.calls[-1] == ("view",)
    # another loss and back: Python's state follows, the C loss is set as for every named loss
    env.handle.calls.clear()
    learner.set_loss("policy", "awr", temperature=2.0)
    learner.step(batch)
    assert env.handle.calls == [("loss", 0, _lib.GS_LOSS_AWR), ("step", 1, 33), ("step", 5, 33), ("step", 0, 33), ("step", 6, 33)]
    env.handle.calls.clear()
    learner.set_loss("policy", "pathwise", alpha=0.5, pathwise_stochastic=False)
    assert env.handle.calls == [("loss", 0, _lib.GS_LOSS_DEFAULT)]
    got = learner.loss("policy")
    assert (got["name"], got["alpha"], got["bc_coef"], got["stochastic"], got["seed"]) == ("pathwise", 0.5, 0.0, False, 0)
    # explicit use on a learner whose policy_loss is something else
    env = _Env()
    plain = DeviceLearner(env, nets=("policy",))
    assert plain.loss("policy")["name"] == "ppo"
    env.handle.calls.clear()
    plain.step_pathwise(batch, alpha=0.1)
    plain.step(batch)
    assert env.handle.calls == [("pathwise", 33, 0.1, 0.0, 1, 0, 0, 40), ("step", 0, 33)]
    for kw in (dict(alpha=-1.0), dict(bc_coef=math.nan), dict(alpha=math.inf), dict(stochastic=2), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5),
               dict(draw=-1), dict(draw=2 ** 32), dict(draw=True)):
        with pytest.raises(ValueError):
            plain.step_pathwise(batch, **kw)
    with pytest.raises(ValueError):
        DeviceLearner(_Env(), nets=("value",)).step_pathwise(batch)
    with pytest.raises(ValueError):
        DeviceLearner(_Env(), nets=("value",)).pathwise_views()
    with pytest.raises(ValueError):
        learner.set_loss("value", "pathwise")


@pytest.mark.parametrize("kw", [dict(nets=("value", "q1"), policy_loss="pathwise"), dict(policy_loss="pathwise", alpha=-0.1),
                                dict(policy_loss="pathwise", alpha=math.nan), dict(policy_loss="pathwise", bc_coef=math.inf),
                                dict(policy_loss="pathwise", bc_coef=-2.0), dict(policy_loss="pathwise", pathwise_stochastic=1),
                                dict(policy_loss="pathwise", pathwise_seed=-3), dict(policy_loss="pathwise", pathwise_seed=2 ** 64),
                                dict(alpha=-0.1), dict(bc_coef=math.nan), dict(value_loss="pathwise"), dict(nets=("q1",), q_loss="pathwise")])
def test_device_learner_refuses_before_anything_is_created(kw):
    env = _Env()
    with pytest.raises(ValueError):
        DeviceLearner(env, **kw)
    assert env.handle.calls == []
