"""CPU-only: the NumPy restatements of the device learner (grid_fed_rl_gym_amd/learner.py; include/gridstep.h "the learner") against
torch on the CPU, and the host logic of ``DeviceLearner``.

``ppo_grad_np(exact=True)`` / ``value_grad_np(exact=True)`` against torch autograd in float64 on the same float32-rounded operands,
with the loss of examples/device_ppo_update.py: both sides are float64 and differ in summation order only, so rtol 1e-10 and
atol 1e-12 max|g| per tensor.  ``adam_np`` over three steps against ``torch.optim.Adam`` in float32 (behind ``clip_grad_norm_``
where ``max_grad_norm`` is on): the roundings are of the same kind but not pinned bit for bit against torch, so rtol 1e-6."""
import math

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import DeviceLearner, adam_np, ppo_grad_np, split_parameters, value_grad_np

torch = pytest.importorskip("torch")

N, D, A = 185, 71, 4
ACT = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}


def _layers(dims, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    ws = [(rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) + shift).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]).astype(np.float32) for l in range(len(dims) - 1)]
    return list(zip(ws, bs))


def _forward64(layers, x, activation):
    x = x.astype(np.float64)
    for l, (w, b) in enumerate(layers):
        x = x @ w.astype(np.float64).T + b.astype(np.float64)
        if l < len(layers) - 1:
            x = np.maximum(x, 0) if activation == "relu" else np.tanh(x) if activation == "tanh" else np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    return x


def _rollout(layers, activation, seed):
    """observations, the policy's own sampled actions, their log-probabilities (the device's formula) and advantages"""
    rng = np.random.default_rng(seed)
    obs = rng.normal(0.0, 1.0, (N, layers[0][0].shape[1])).astype(np.float32)
    out = _forward64(layers, obs, activation)
    a_dim = out.shape[1] // 2
    ls = np.clip(out[:, a_dim:], -20.0, 2.0)
    eps = rng.normal(0.0, 1.0, (N, a_dim))
    act = np.tanh(out[:, :a_dim] + np.exp(ls) * eps)
    lp = ((-0.5 * eps * eps - ls) - 0.5 * math.log(2.0 * math.pi) - np.log(1.0 - act * act + 1e-6)).sum(axis=1)
    return obs, act, lp, rng.normal(0.0, 1.0, N)


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


def _torch_ppo(layers, activation, obs, act, lp_old, adv, clip, ent_coef):
    actor = _module(layers, activation)
    obs_t, actions = torch.from_numpy(obs.astype(np.float64)), torch.from_numpy(act)
    mean, log_std_raw = torch.chunk(actor(obs_t), 2, dim=-1)
    log_std = torch.clamp(log_std_raw, -20.0, 2.0)
    x = torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7))
    eps = (x - mean) * torch.exp(-log_std)
    lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)
    ratio = torch.exp(lp - torch.from_numpy(lp_old))
    adv_t = torch.from_numpy(adv)
    surr = torch.min(ratio * adv_t, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_t)
    entropy = (log_std + 0.5 * math.log(2.0 * math.pi * math.e)).sum(dim=-1)
    loss = -surr.mean() - ent_coef * entropy.mean()
    loss.backward()
    lins = [m for m in actor if hasattr(m, "weight")]
    return float(loss.detach()), lp.detach().numpy(), ratio.detach().numpy(), [(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lins], log_std_raw.detach().numpy()


def _close(got, want, what):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    assert got.shape == want.shape, what
    assert np.allclose(got, want, rtol=1e-10, atol=1e-12 * scale), (what, float(np.max(np.abs(got - want))), scale)


# name: (hidden widths, activation, ent_coef, bias added to the log_std half of the last layer or None)
PPO_CASES = {
    "relu-64x64": ([64, 64], "relu", 0.0, None),
    "tanh-64x64-entropy": ([64, 64], "tanh", 0.01, None),
    "elu-64x64": ([64, 64], "elu", 0.0, None),
    "single-layer": ([], "relu", 0.0, None),
    "four-layers": ([64, 48, 64], "relu", 0.003, None),
    "width-40": ([40, 40], "tanh", 0.0, None),
    "clamped-log-std": ([64, 64], "relu", 0.02, (3.5, -24.0)),
}


@pytest.mark.parametrize("name", sorted(PPO_CASES))
def test_ppo_gradient_matches_torch_autograd_in_float64(name):
    hidden, activation, ent_coef, clamp = PPO_CASES[name]
    dims = [D] + hidden + [2 * A]
    behaviour = _layers(dims, 0)
    if clamp is not None:            # log_std biases beyond +2 and below -20: the clamp's gradient is zero there
        behaviour[-1][1][A] += clamp[0]; behaviour[-1][1][A + 1] += clamp[1]
    obs, act, lp_old, adv = _rollout(behaviour, activation, 5)
    # the parameters move after the rollout, so that ratios leave 1 and some samples are clipped
    current = [((w + np.float32(0.003)).astype(np.float32), b.copy()) for w, b in behaviour]
    res = ppo_grad_np(current, obs, act, lp_old, adv, 0.2, ent_coef, exact=True, activation=activation)
    loss, lp, ratio, grads, lsr = _torch_ppo(current, activation, obs, act, lp_old, adv, 0.2, ent_coef)
    assert res["clipped"].sum() >= 1 and res["clipped"].sum() < N // 2, res["clipped"].sum()
    if clamp is not None:
        outside = (lsr > 2.0) | (lsr < -20.0)
        assert outside[:, 0].all() and outside[:, 1].all() and np.array_equal(res["log_std_outside"], outside)
        assert all(np.all(g[1][A:A + 2] == 0.0) for g in [res["grads"][-1], grads[-1]])
    _close(res["log_probs_new"], lp, "log_probs_new")
    _close(res["ratio"], ratio, "ratio")
    assert abs(res["loss"] - loss) <= 1e-10 * abs(loss) + 1e-12
    for l, ((gw, gb), (tw, tb)) in enumerate(zip(res["grads"], grads)):
        assert gw.dtype == np.float64
        _close(gw, tw, f"dW{l}"); _close(gb, tb, f"db{l}")
    # the float32 evaluation lies near the exact one, and flags given from outside are used
    f32 = ppo_grad_np(current, obs, act, lp_old, adv, 0.2, ent_coef, activation=activation, clipped=res["clipped"])
    assert f32["grads"][0][0].dtype == np.float32
    for (gw, gb), (ew, eb) in zip(f32["grads"], res["grads"]):
        assert np.max(np.abs(gw - ew)) <= 1e-4 * max(np.max(np.abs(ew)), 1e-30)
    none = ppo_grad_np(current, obs, act, lp_old, adv, 0.2, 0.0, exact=True, activation=activation, clipped=np.ones(N, dtype=np.int32))
    if clamp is None:
        assert all(np.all(gw == 0.0) and np.all(gb == 0.0) for gw, gb in none["grads"])


@pytest.mark.parametrize("hidden,activation", [([64, 64], "relu"), ([40, 40], "tanh"), ([64, 64], "elu"), ([], "relu"), ([64, 48, 64], "elu")])
def test_value_gradient_matches_torch_autograd_in_float64(hidden, activation):
    layers = _layers([D] + hidden + [1], 3)
    rng = np.random.default_rng(9)
    obs, ret = rng.normal(0.0, 1.0, (N, D)).astype(np.float32), rng.normal(0.0, 2.0, N).astype(np.float32)
    res = value_grad_np(layers, obs, ret, exact=True, activation=activation)
    critic = _module(layers, activation)
    v = critic(torch.from_numpy(obs.astype(np.float64)))[:, 0]
    loss = ((v - torch.from_numpy(ret.astype(np.float64))) ** 2).mean()
    loss.backward()
    assert abs(res["loss"] - float(loss.detach())) <= 1e-10 * float(loss.detach())
    _close(res["values"], v.detach().numpy(), "values")
    lins = [m for m in critic if hasattr(m, "weight")]
    for l, ((gw, gb), m) in enumerate(zip(res["grads"], lins)):
        _close(gw, m.weight.grad.numpy(), f"dW{l}"); _close(gb, m.bias.grad.numpy(), f"db{l}")


@pytest.mark.parametrize("weight_decay,max_grad_norm", [(0.0, 0.0), (1e-5, 0.0), (0.0, 0.5), (1e-2, 0.5)])
def test_adam_np_follows_torch_adam_in_float32(weight_decay, max_grad_norm):
    rng = np.random.default_rng(4)
    shapes = [(64, 71), (64,), (8, 64), (8,)]
    cfg = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    # magnitudes in [0.1, 0.5]: p - step * (m / denom) is a difference, and a relative tolerance on it says something only away from
    # cancellation -- a rounding of the update (3e-3 x 2^-24) is 1e-6 of a parameter of 2e-4; three steps move a parameter by < 0.01
    ps = [(rng.uniform(0.1, 0.5, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32) for s in shapes]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.Adam(tp, lr=cfg["lr"], betas=cfg["betas"], eps=cfg["eps"], weight_decay=weight_decay)
    ms, vs = [np.zeros(s, np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes]
    for t in range(1, 4):
        gs = [rng.normal(0.0, 1.0, s).astype(np.float32) for s in shapes]
        norm = math.sqrt(math.fsum(float(x) * float(x) for g in gs for x in g.ravel()))
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g.copy())
        if max_grad_norm > 0.0:
            torch.nn.utils.clip_grad_norm_(tp, max_grad_norm)
        opt.step()
        for k in range(len(ps)):
            ps[k], ms[k], vs[k] = adam_np(ps[k], gs[k], ms[k], vs[k], t, cfg, norm)
            assert ps[k].dtype == np.float32 and ms[k].dtype == np.float32 and vs[k].dtype == np.float32
        for p, q in zip(ps, tp):
            assert np.allclose(p, q.detach().numpy(), rtol=1e-6, atol=0.0), (t, float(np.max(np.abs(p - q.detach().numpy()))))
    if max_grad_norm > 0.0:
        assert norm > max_grad_norm          # the clip was active


def test_split_parameters_is_torch_order():
    dims = [5, 3, 2]
    flat = np.arange(3 * 6 + 2 * 4, dtype=np.float32)
    W, b = split_parameters(flat, dims)
    assert np.array_equal(W[0], flat[:15].reshape(3, 5)) and np.array_equal(b[0], flat[15:18])
    assert np.array_equal(W[1], flat[18:24].reshape(2, 3)) and np.array_equal(b[1], flat[24:26])
    with pytest.raises(ValueError):
        split_parameters(flat[:-1], dims)


class _FakeHandle:
    def __init__(self):
        self.created, self.steps = [], []

    def learner_create(self, net, cfg):
        self.created.append((net, cfg))

    def learner_step(self, net, batch, n, stream):
        self.steps.append((net, n))


class _FakeEnv:
    def __init__(self):
        self.handle = _FakeHandle()


def test_device_learner_names_and_argument_rules():
    assert [_lib.learner_net(k) for k in ("policy", "value", "voltage", "frequency", "thermal")] == [0, 1, 2, 3, 4]
    assert _lib.learner_net(3) == 3
    for bad in ("critic", "Voltage", 5, -1):
        with pytest.raises(ValueError):
            _lib.learner_net(bad)
    env = _FakeEnv()
    learner = DeviceLearner(env, nets=("policy", "value", "thermal"), lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-5, clip=0.1,
                            ent_coef=0.01, max_grad_norm=0.5)
    assert [net for net, _ in env.handle.created] == [0, 1, 4]
    cfg = env.handle.created[0][1]
    assert cfg.struct_size == 72 and (cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.weight_decay, cfg.max_grad_norm, cfg.clip, cfg.ent_coef) == \
        (1e-3, 0.8, 0.99, 1e-7, 1e-5, 0.5, 0.1, 0.01)
    learner.step(dict(observations=np.zeros((12, 3), np.float32)))
    assert env.handle.steps == [(0, 12), (1, 12), (4, 12)]
    with pytest.raises(ValueError):
        learner.stats("voltage")             # not one of this learner's networks
    with pytest.raises(ValueError):
        learner.value("policy")
    assert DeviceLearner(_FakeEnv(), nets="value").nets == ("value",)
    rules = [dict(nets=()), dict(nets=("policy", "policy")), dict(nets=("policy", "q")), dict(lr=-1.0), dict(lr=float("nan")), dict(betas=(1.0, 0.9)),
             dict(betas=(0.9,)), dict(betas=(0.9, -0.1)), dict(eps=float("inf")), dict(weight_decay=-1e-3), dict(clip=-0.2), dict(max_grad_norm=-1.0),
             dict(ent_coef=float("nan"))]
    for kw in rules:
        fresh = _FakeEnv()
        with pytest.raises(ValueError):
            DeviceLearner(fresh, **kw)
        assert fresh.handle.created == [], kw          # refused before anything reaches the handle
