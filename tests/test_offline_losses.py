"""CPU-only: the NumPy restatements of the offline losses (grid_fed_rl_gym_amd/learner.py; include/gridstep.h "the learner's loss";
DESIGN.md section 21) against torch on the CPU, their stated consequences, and the host logic of ``DeviceLearner``'s new arguments.

``awr_grad_np(exact=True)`` / ``expectile_grad_np(exact=True)`` against torch autograd in float64 on the same float32-rounded
operands: both sides are float64 and differ in summation order only, so section 19's rtol 1e-10 and atol 1e-12 max|g| per tensor.
Shapes 71 -> 64 -> 64 -> 8 (A = 4), n = 185."""
import math

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import DeviceLearner, awr_grad_np, expectile_grad_np, value_grad_np

torch = pytest.importorskip("torch")

N, D, A = 185, 71, 4
ACT = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}
INF = math.inf


def _layers(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]).astype(np.float32) for l in range(len(dims) - 1)]
    return list(zip(ws, bs))


def _dataset(seed):
    """observations, actions of some OTHER behaviour (uniform, as a random-action rollout stores them) and advantages"""
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (N, D)).astype(np.float32), rng.uniform(-1.0, 1.0, (N, A)), rng.normal(0.0, 1.0, N).astype(np.float32)


def _module(layers, activation):
    mods = []
    for l, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.astype(np.float64))); lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        mods.append(lin)
        if l < len(layers) - 1:
            mods.append(ACT[activation]())
    return torch.nn.Sequential(*mods)


def _torch_awr(layers, activation, obs, act, adv, temperature, weight_max, ent_coef):
    actor = _module(layers, activation)
    actions = torch.from_numpy(act)
    mean, log_std_raw = torch.chunk(actor(torch.from_numpy(obs.astype(np.float64))), 2, dim=-1)
    log_std = torch.clamp(log_std_raw, -20.0, 2.0)
    x = torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7))
    eps = (x - mean) * torch.exp(-log_std)
    lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)
    w = torch.clamp(torch.exp(torch.from_numpy(adv.astype(np.float64)) / temperature), max=weight_max)      # (a constant: no graph behind it)
    entropy = (log_std + 0.5 * math.log(2.0 * math.pi * math.e)).sum(dim=-1)
    loss = -(w * lp).mean() - ent_coef * entropy.mean()
    loss.backward()
    lins = [m for m in actor if hasattr(m, "weight")]
    return float(loss.detach()), lp.detach().numpy(), w.numpy(), [(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lins], log_std_raw.detach().numpy()


def _close(got, want, what):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    assert got.shape == want.shape, what
    assert np.allclose(got, want, rtol=1e-10, atol=1e-12 * scale), (what, float(np.max(np.abs(got - want))), scale)


# name: (activation, ent_coef, temperature, weight_max, biases added to log_std 0 and 1 or None)
AWR_CASES = {
    "relu": ("relu", 0.0, 1.0, 20.0, None),
    "tanh-entropy": ("tanh", 0.01, 0.5, 20.0, None),
    "elu": ("elu", 0.0, 2.0, INF, None),
    "capped-and-uncapped": ("relu", 0.003, 0.7, 1.5, None),
    "clamped-log-std": ("relu", 0.02, 1.0, 20.0, (3.5, -24.0)),
    "behaviour-cloning": ("tanh", 0.0, INF, INF, None),
}


@pytest.mark.parametrize("name", sorted(AWR_CASES))
def test_awr_gradient_matches_torch_autograd_in_float64(name):
    activation, ent_coef, temperature, weight_max, clamp = AWR_CASES[name]
    layers = _layers([D, 64, 64, 2 * A], 0)
    if clamp is not None:            # log_std biases beyond +2 and below -20: the clamp's gradient is zero there
        layers[-1][1][A] += clamp[0]; layers[-1][1][A + 1] += clamp[1]
    obs, act, adv = _dataset(5)
    res = awr_grad_np(layers, obs, act, adv, temperature, weight_max, ent_coef, exact=True, activation=activation)
    loss, lp, w, grads, lsr = _torch_awr(layers, activation, obs, act, adv, temperature, weight_max, ent_coef)
    if name == "capped-and-uncapped":
        assert 1 <= res["capped"].sum() < N
        assert np.all(res["weights"][res["capped"] == 1] == weight_max) and np.all(res["weights"][res["capped"] == 0] <= weight_max)
        assert res["clip_fraction"] == res["capped"].sum() / N
    if math.isinf(weight_max):
        assert not res["capped"].any()
    if clamp is not None:
        outside = (lsr > 2.0) | (lsr < -20.0)
        assert outside[:, 0].all() and outside[:, 1].all() and np.array_equal(res["log_std_outside"], outside)
        assert all(np.all(g[1][A:A + 2] == 0.0) for g in [res["grads"][-1], grads[-1]])
    _close(res["log_probs_new"], lp, "log_probs_new")
    _close(res["weights"], w, "weights")
    _close(res["loss_terms"], w * lp, "loss_terms")
    assert abs(res["loss"] - loss) <= 1e-10 * abs(loss) + 1e-12
    assert math.isnan(res["approx_kl"])
    for l, ((gw, gb), (tw, tb)) in enumerate(zip(res["grads"], grads)):
        assert gw.dtype == np.float64
        _close(gw, tw, f"dW{l}"); _close(gb, tb, f"db{l}")
    # the float32 evaluation lies near the exact one, and flags given from outside are used
    f32 = awr_grad_np(layers, obs, act, adv, temperature, weight_max, ent_coef, activation=activation, capped=res["capped"])
    assert f32["grads"][0][0].dtype == np.float32
    for (gw, gb), (ew, eb) in zip(f32["grads"], res["grads"]):
        assert np.max(np.abs(gw - ew)) <= 1e-4 * max(np.max(np.abs(ew)), 1e-30)
    if math.isfinite(weight_max) and ent_coef == 0.0:
        # every sample flagged: every weight is weight_max, so the gradient is weight_max times behaviour cloning's
        every = awr_grad_np(layers, obs, act, adv, temperature, weight_max, 0.0, exact=True, activation=activation, capped=np.ones(N, np.int32))
        cloning = awr_grad_np(layers, obs, act, adv, INF, INF, 0.0, exact=True, activation=activation)
        for (gw, gb), (cw, cb) in zip(every["grads"], cloning["grads"]):
            _close(gw, weight_max * cw, "all capped"); _close(gb, weight_max * cb, "all capped")
    lp_old = res["log_probs_new"] + 0.25
    kl = awr_grad_np(layers, obs, act, adv, temperature, weight_max, ent_coef, exact=True, activation=activation, lp_old=lp_old)["approx_kl"]
    assert kl == math.fsum(lp_old - res["log_probs_new"]) / N


def test_behaviour_cloning_is_the_gradient_of_minus_mean_log_probability():
    layers = _layers([D, 64, 64, 2 * A], 2)
    obs, act, adv = _dataset(7)
    res = awr_grad_np(layers, obs, act, adv, INF, INF, 0.0, exact=True)
    assert np.all(res["weights"] == 1.0) and not res["capped"].any()          # A / inf = 0 and exp(0) = 1: exactly
    assert np.array_equal(res["loss_terms"], res["log_probs_new"])
    actor = _module(layers, "relu")
    actions = torch.from_numpy(act)
    mean, log_std_raw = torch.chunk(actor(torch.from_numpy(obs.astype(np.float64))), 2, dim=-1)
    log_std = torch.clamp(log_std_raw, -20.0, 2.0)
    eps = (torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7)) - mean) * torch.exp(-log_std)
    lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)
    (-lp.mean()).backward()
    assert abs(res["loss"] + float(lp.mean().detach())) <= 1e-10 * abs(res["loss"])
    lins = [m for m in actor if hasattr(m, "weight")]
    for l, ((gw, gb), m) in enumerate(zip(res["grads"], lins)):
        _close(gw, m.weight.grad.numpy(), f"dW{l}"); _close(gb, m.bias.grad.numpy(), f"db{l}")


def test_a_tiny_temperature_with_the_cap_on_gives_finite_weights():
    layers = _layers([D, 64, 64, 2 * A], 2)
    obs, act, adv = _dataset(7)
    assert adv.max() > 1.0 and adv.min() < -1.0
    for exact in (True, False):
        res = awr_grad_np(layers, obs, act, adv, 1e-3, 20.0, 0.0, exact=exact)          # exp(A / 1e-3) overflows float64 for A > 0.71
        assert np.all(np.isfinite(res["weights"])) and np.all(res["weights"] <= 20.0) and res["weights"].max() == 20.0
        assert res["capped"].sum() >= 1 and np.all(res["weights"][res["capped"] == 1] == 20.0)
        assert all(np.all(np.isfinite(gw)) and np.all(np.isfinite(gb)) for gw, gb in res["grads"]) and math.isfinite(res["loss"])


@pytest.mark.parametrize("activation", ["relu", "tanh", "elu"])
@pytest.mark.parametrize("tau", [0.1, 0.7])
def test_expectile_gradient_matches_torch_autograd_in_float64(activation, tau):
    layers = _layers([D, 64, 64, 1], 3)
    rng = np.random.default_rng(9)
    obs, ret = rng.normal(0.0, 1.0, (N, D)).astype(np.float32), rng.normal(0.0, 2.0, N).astype(np.float32)
    res = expectile_grad_np(layers, obs, ret, tau, exact=True, activation=activation)
    assert 1 <= res["below"].sum() < N          # both signs of v - ret
    critic = _module(layers, activation)
    v = critic(torch.from_numpy(obs.astype(np.float64)))[:, 0]
    diff = torch.from_numpy(ret.astype(np.float64)) - v          # the reference's sign: weight tau where diff > 0
    weight = torch.where(diff > 0, torch.full_like(diff, tau), torch.full_like(diff, 1.0 - tau))
    loss = (weight * diff ** 2).mean()
    loss.backward()
    assert abs(res["loss"] - float(loss.detach())) <= 1e-10 * float(loss.detach())
    _close(res["values"], v.detach().numpy(), "values")
    lins = [m for m in critic if hasattr(m, "weight")]
    for l, ((gw, gb), m) in enumerate(zip(res["grads"], lins)):
        _close(gw, m.weight.grad.numpy(), f"dW{l}"); _close(gb, m.bias.grad.numpy(), f"db{l}")


@pytest.mark.parametrize("exact", [True, False])
def test_expectile_at_one_half_is_exactly_half_of_the_mean_squared_error(exact):
    layers = _layers([D, 64, 64, 1], 3)
    rng = np.random.default_rng(9)
    obs, ret = rng.normal(0.0, 1.0, (N, D)).astype(np.float32), rng.normal(0.0, 2.0, N).astype(np.float32)
    half, mse = expectile_grad_np(layers, obs, ret, 0.5, exact=exact), value_grad_np(layers, obs, ret, exact=exact)
    assert np.array_equal(half["loss_terms"], 0.5 * mse["loss_terms"]) and half["loss"] == 0.5 * mse["loss"]
    # the head gradient is half of the other's bit for bit (a product with 0.5 is exact), and the last bias gradient is its sum
    assert np.array_equal(half["grads"][-1][1], (0.5 * mse["grads"][-1][1]).astype(half["grads"][-1][1].dtype))
    if exact:          # float64 throughout: halving commutes with every product and sum of the backward pass
        for (hw, hb), (mw, mb) in zip(half["grads"], mse["grads"]):
            assert np.array_equal(hw, 0.5 * mw) and np.array_equal(hb, 0.5 * mb)


def test_cap_at_a_midpoint_of_order_statistics_separates_the_samples():
    """the construction tests/test_gpu_offline_losses.py uses for ``weight_max``, on synthetic advantages: the geometric midpoint of
    two adjacent order statistics of exp(A / temperature) that lie more than 2e-4 apart leaves no sample within 1e-4 of the cap"""
    rng = np.random.default_rng(1)
    adv = rng.normal(0.0, 1.0, 185).astype(np.float32)
    adv[90:100] = adv[90]                       # ties around the median: the pair moves on
    u = np.sort(np.exp(adv.astype(np.float64) / 0.7))
    k = len(u) // 2
    while not u[k + 1] > u[k] * (1.0 + 2e-4):
        k += 1
    cap = math.sqrt(u[k] * u[k + 1])
    layers = _layers([D, 64, 64, 2 * A], 0)
    obs, act, _ = _dataset(5)
    res = awr_grad_np(layers, obs, act, adv, 0.7, cap, 0.0, exact=True)
    band = np.abs(np.exp(adv.astype(np.float64) / 0.7) - cap) <= 1e-4 * cap
    assert not band.any() and res["capped"].sum() == len(u) - 1 - k and 1 <= res["capped"].sum() < 185


class _FakeHandle:
    def __init__(self):
        self.created, self.losses = [], []

    def learner_create(self, net, cfg):
        self.created.append((net, cfg))

    def learner_set_loss(self, net, loss):
        self.losses.append((net, loss.kind, loss.temperature, loss.weight_max, loss.expectile))


class _FakeEnv:
    def __init__(self):
        self.handle = _FakeHandle()


def test_device_learner_loss_arguments():
    assert (_lib.GS_LOSS_DEFAULT, _lib.GS_LOSS_AWR, _lib.GS_LOSS_EXPECTILE) == (0, 1, 2)
    assert _lib.learner_loss("awr").struct_size == 32
    env = _FakeEnv()
    DeviceLearner(env, nets=("policy", "value", "thermal"))          # the defaults never reach the new entry
    assert env.handle.losses == [] and len(env.handle.created) == 3
    env = _FakeEnv()
    learner = DeviceLearner(env, nets=("policy", "value", "thermal"), policy_loss="awr", temperature=0.5, weight_max=10.0, value_loss="expectile",
                            expectile=0.8)
    assert env.handle.losses == [(0, 1, 0.5, 10.0, 0.0), (1, 2, 0.0, 0.0, 0.8), (4, 2, 0.0, 0.0, 0.8)]
    env = _FakeEnv()
    learner = DeviceLearner(env, nets=("policy", "value"), policy_loss="bc")
    assert env.handle.losses == [(0, 1, INF, INF, 0.0)]
    learner.set_loss("policy", "awr", temperature=INF, weight_max=3.0)
    learner.set_loss("value", "expectile", expectile=0.25)
    learner.set_loss("policy", "ppo")
    assert env.handle.losses[1:] == [(0, 1, INF, 3.0, 0.0), (1, 2, 0.0, 0.0, 0.25), (0, 0, 0.0, 0.0, 0.0)]
    rules = [dict(policy_loss="iql"), dict(policy_loss="expectile"), dict(value_loss="awr"), dict(value_loss="huber"),
             dict(policy_loss="awr", temperature=0.0), dict(policy_loss="awr", temperature=-1.0), dict(policy_loss="awr", temperature=float("nan")),
             dict(policy_loss="awr", weight_max=0.0), dict(policy_loss="awr", weight_max=-INF), dict(policy_loss="awr", weight_max=float("nan")),
             dict(value_loss="expectile", expectile=0.0), dict(value_loss="expectile", expectile=1.0), dict(value_loss="expectile", expectile=float("nan")),
             dict(nets=("value",), policy_loss="iql"), dict(nets=("policy",), value_loss="expectile", expectile=1.5)]
    for kw in rules:
        fresh = _FakeEnv()
        with pytest.raises(ValueError):
            DeviceLearner(fresh, **kw)
        assert fresh.handle.created == [] and fresh.handle.losses == [], kw          # refused before anything reaches the handle
    n_before = len(env.handle.losses)
    for call in (lambda: learner.set_loss("policy", "expectile"), lambda: learner.set_loss("value", "awr"), lambda: learner.set_loss("policy"),
                 lambda: learner.set_loss("thermal", "mse"), lambda: learner.set_loss("policy", "awr", temperature=0.0),
                 lambda: learner.set_loss("value", "expectile", expectile=-0.1), lambda: awr_grad_np([], [], [], [], 0.0, 1.0, 0.0),
                 lambda: awr_grad_np([], [], [], [], 1.0, float("nan"), 0.0), lambda: expectile_grad_np([], [], [], 1.0)):
        with pytest.raises(ValueError):
            call()
    assert len(env.handle.losses) == n_before
    with pytest.raises(ValueError):
        _lib.learner_loss("huber")
