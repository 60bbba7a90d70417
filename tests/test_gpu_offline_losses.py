"""GPU: the learner's offline losses (include/gridstep.h "the learner's loss") -- ``gs_learner_step`` under
GS_LOSS_AWR and GS_LOSS_EXPECTILE against ``awr_grad_np`` / ``expectile_grad_np`` of grid_fed_rl_gym_amd/learner.py: gradients, cap
flags, weights, per-sample arrays, statistics, Adam bit for bit, the entry's rules and lifetime, and non-interference.

Set-up copied from tests/test_gpu_learner.py: ``episode_length`` 7, a float32 Gaussian policy, the reward critic and cost critics on
voltage and thermal, the normalisation from a short random rollout; T = 37 steps of B = 5 instances (N = 185).  The dataset is what an
offline client holds: a RANDOM-ACTION rollout with the policy installed but not acting (no log-probabilities recorded).  It is
evaluated with lam = 1 and no bootstrap at episode ends (Monte-Carlo returns), and the reward critic's last bias is moved to the median
return before the evaluation that counts: v - ret then has both signs (asserted), and so has the advantage.  One case ("ieee13-elu")
adds 3.5 to one log_std bias, beyond the clamp's upper end (asserted); one is the 123-bus feeder with hidden 256, 256 and A = 8.

Bounds, none of them computed from the device (section 19's, with its two amendments):
  gradients, log_probs_new   within 4 E_ref, E_ref = the float32 restatement's error against ``exact=True`` per tensor; at n = 1 from 32
                             single rows, for one-entry tensors at least the float32 rounding of the terms.  The device's cap flags are
                             fed to both restatements.
  cap flags                  equal to the exact restatement's outside a relative band of 1e-4 around weight_max; at most 2 % of a
                             minibatch inside the band.  Met by construction: weight_max is the geometric midpoint of two adjacent order
                             statistics of exp(A / temperature) near the median that lie more than 2e-4 apart (``_cap``).
  weights                    fmin(exp(A / temperature), weight_max) of the device's own inputs at rtol 1e-15 (two exps, each correct to an ulp)
  statistics                 section 17's order: |mean^ - mean| <= (d + 2) 2^-53 sum|x| / n, d = ceil(n / 1024) - 1 + 10, against
                             ``math.fsum`` over the device's own per-sample arrays
  Adam, lifetime, twins      bit-equal.
Temperature: 1 under GS_ADVNORM_ROLLOUT (unit-variance advantages); under GS_ADVNORM_NONE the standard deviation of the rollout's raw
advantages, so that A / temperature has the same spread."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.federated import fedavg_np
from grid_fed_rl_gym_amd.learner import adam_np, awr_grad_np, expectile_grad_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, rollout_device

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
B, T = 5, 37
# name: (feeder, hidden widths, activation, added to the bias of log_std 0)
CASES = {
    "ieee13-relu": ("ieee13", [64, 64], "relu", 0.0),
    "ieee13-elu": ("ieee13", [64, 64], "elu", 3.5),
    "ieee123-relu": ("ieee123", [256, 256], "relu", 0.0),
}
CHANNELS = {"voltage": 0, "thermal": 2}
NETS = ("policy", "value", "thermal")
ENT, TAU = 0.01, 0.7
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, clip=0.2, ent_coef=ENT, max_grad_norm=0.5)
OFFLINE = dict(policy_loss="awr", temperature=1.0, weight_max=20.0, value_loss="expectile", expectile=TAU)
FIELDS = ["observations", "actions", "advantages", "returns", "values", "indices", "cost_returns"]
U = 2.0 ** -53
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
INF = math.inf
WORST = {}
MISSED = []


def _env(feeder, num_envs=B):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=num_envs, solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=7)


_NORM = {}


def _normalisation(feeder):
    if feeder not in _NORM:
        env = _env(feeder, 64)
        obs = P.collect_random_data(env, 4, seed=11)["observations"]
        env.close()
        mean, std = obs.mean(axis=0), obs.std(axis=0)
        constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
        _NORM[feeder] = (mean, np.where(constant, 1.0, std + 1e-6))
    return _NORM[feeder]


def _layers(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


def _networks(env, feeder, hidden, activation, ls_bias):
    mean, std = _normalisation(feeder)
    A = env.action_dim
    ws, bs = _layers([env.obs_dim] + hidden + [2 * A], 1)
    bs[-1][A] += ls_bias
    pol = P.MLPPolicy(ws, bs, activation=activation, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    raw = {name: _layers([env.obs_dim] + hidden + [1], seed) for name, seed in (("value", 2), ("voltage", 10), ("thermal", 12))}
    return pol, raw


def _value(c, name, shift=0.0):
    ws, bs = c["raw"][name]
    bs = [b.copy() for b in bs]
    bs[-1][0] += shift
    mean, std = _normalisation(c["feeder"])
    return P.MLPValue(ws, bs, activation=c["activation"], obs_mean=mean, obs_std=std)


def _install(c):
    """the networks as first installed: ends every learner of the handle"""
    env = c["env"]
    env.set_policy(c["pol"], stochastic=True)
    env.set_value(c["vals"]["value"])
    for name in CHANNELS:
        env.set_cost_value(name, c["vals"][name])


def _evaluate(c):
    env = c["env"]
    P.evaluate_rollout(env, gamma=0.99, lam=1.0, bootstrap=())
    P.rollout_costs(env, P.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5), kinds="excess")
    P.evaluate_rollout_costs(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))


def _build(name, collect="random"):
    """``collect``: "random" (uniform actions drawn on the device), "policy" (the stochastic policy acts: log-probabilities are
    recorded) or an array [T, B, A] of uploaded actions"""
    feeder, hidden, activation, ls_bias = CASES[name]
    env = _env(feeder)
    pol, raw = _networks(env, feeder, hidden, activation, ls_bias)
    c = dict(env=env, pol=pol, raw=raw, feeder=feeder, activation=activation)
    c["vals"] = {k: _value(c, k) for k in raw}
    _install(c)
    env.reset(seed=3)
    if isinstance(collect, str):
        rollout_device(env, T, seed=7, reset=False, policy=True if collect == "policy" else None)
    else:
        rollout_device(env, T, reset=False, actions=collect)
    stochastic = isinstance(collect, str) and collect == "policy"
    h = env.handle
    _evaluate(c)
    ret = h.rollout_onpolicy_download(("returns",))["returns"]
    c["vals"]["value"] = _value(c, "value", float(np.median(ret)))          # v - ret gets both signs
    env.set_value(c["vals"]["value"])
    _evaluate(c)
    fields = FIELDS + (["log_probs"] if stochastic else [])
    c["batches"] = {adv: OnPolicyBatches(env, B * T, policy=pol, adv_norm=adv, seed=5, fields=fields) for adv in ("rollout", "none")}
    c["batches"]["rollout"].prepare()
    c["actions"] = h.rollout_download(want=("actions",))["actions"].reshape(B * T, -1)
    c["logp"] = h.rollout_onpolicy_download(("log_probs",))["log_probs"].reshape(B * T) if stochastic else None
    c["adv_std"] = float(h.rollout_onpolicy_download(("advantages",))["advantages"].std())
    return c


_PREPARED = {}


@pytest.fixture(scope="module")
def prepared():
    def get(name, collect="random"):
        if (name, collect) not in _PREPARED:
            _PREPARED[(name, collect)] = _build(name, collect)
        return _PREPARED[(name, collect)]
    yield get
    for c in _PREPARED.values():
        c["env"].close()
    _PREPARED.clear()
    print("largest device error / E_ref:", {k: round(v, 3) for k, v in WORST.items()})


def _host(batch):
    out = {}
    for k, v in batch.items():
        out[k] = [None if x is None else x.to_host() for x in v] if isinstance(v, list) else v.to_host()
    return out


def _pairs(W, b):
    return list(zip(W, b))


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


def _within(tag, what, got, exact, f32, rel_ref=None, floor=None):
    """section 19's bound with its two amendments (tests/test_gpu_learner.py ``_within``): rel_ref at n below a tile of rows, floor for
    a tensor of ONE entry"""
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    if rel_ref is not None:
        e_ref = rel_ref * float(np.max(np.abs(exact)))
    if floor is not None:
        e_ref = max(e_ref, floor)
    ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    WORST[what.split("[")[0]] = max(WORST.get(what.split("[")[0], 0.0), ratio if math.isfinite(ratio) else 1e9)
    if not e_dev <= 4.0 * e_ref:          # (every tensor of the step is looked at before the test fails)
        MISSED.append((tag, what, e_dev, e_ref))


def _single_rows(evaluate):
    """E_ref below 32 rows: per tensor the largest error of the float32 restatement over 32 minibatches of ONE row each, relative to
    the exact tensor's largest entry (tests/test_gpu_learner.py ``_single_rows``)"""
    worst = {}
    for j in range(32):
        ex, lo = evaluate(slice(j, j + 1), True), evaluate(slice(j, j + 1), False)
        for l, ((ew, eb), (fw, fb)) in enumerate(zip(ex["grads"], lo["grads"])):
            for what, e, f in ((f"dW[{l}]", ew, fw), (f"db[{l}]", eb, fb)):
                top = float(np.max(np.abs(e)))
                if top > 0.0:
                    worst[what] = max(worst.get(what, 0.0), _err(f, e) / top)
        if "log_probs_new" in ex:
            top = float(np.max(np.abs(ex["log_probs_new"])))
            if top > 0.0:
                worst["log_probs_new"] = max(worst.get("log_probs_new", 0.0), _err(lo["log_probs_new"], ex["log_probs_new"]) / top)
    return worst


def _mean_bound(x, n):
    d = -(-n // 1024) - 1 + 10
    return (d + 2) * U * math.fsum(abs(float(v)) for v in x) / n


def _cap(adv, temperature):
    """weight_max for this minibatch: the geometric midpoint of two adjacent order statistics of exp(A / temperature) near the median
    that lie more than 2e-4 apart relatively (the next pair otherwise); a single sample stays uncapped at twice its weight"""
    u = np.sort(np.exp(np.asarray(adv).astype(np.float64) / temperature))
    if len(u) < 2:
        return 2.0 * float(u[0])
    k = len(u) // 2 - 1
    while k + 1 < len(u) and not u[k + 1] > u[k] * (1.0 + 2e-4):
        k += 1
    assert k + 1 < len(u), "no two order statistics above the median lie 2e-4 apart"
    return math.sqrt(float(u[k]) * float(u[k + 1]))


def _grad_norm_ok(tag, learner, net, st):
    flat = learner.download(net, ("grads",))["grads"]
    norm = math.sqrt(math.fsum(float(x) * float(x) for x in flat))
    assert abs(st["grad_norm"] - norm) <= flat.size * 2.0 ** -52 * norm, (tag, st["grad_norm"], norm)


def _check_awr_step(tag, c, learner, hb, params, n, step, temperature, cap, ent=ENT):
    """one AWR step that has just run on the host batch ``hb`` from the parameters ``params``"""
    idx = hb["indices"]
    act = c["actions"][idx]
    lp_old = None if c["logp"] is None else c["logp"][idx]
    views = {k: v.to_host() for k, v in learner.views("policy").items()}
    dev_flags = views["clipped"]
    layers = _pairs(*params)
    kw = dict(activation=c["activation"])
    adv = hb["advantages"]
    exact = awr_grad_np(layers, hb["observations"], act, adv, temperature, cap, ent, exact=True, capped=dev_flags, lp_old=lp_old, **kw)
    f32 = awr_grad_np(layers, hb["observations"], act, adv, temperature, cap, ent, exact=False, capped=dev_flags, **kw)
    # cap flags: the device's against the exact evaluation's outside a relative band of 1e-4 around weight_max
    u = np.exp(adv.astype(np.float64) / temperature)
    band = np.abs(u - cap) <= 1e-4 * cap
    assert band.sum() <= 0.02 * n, (tag, int(band.sum()))
    assert np.array_equal(dev_flags[~band], exact["capped"][~band]), tag
    print(f"{tag}: capped {int(dev_flags.sum())} of {n}, in the band {int(band.sum())}, log_std outside the clamp {int(exact['log_std_outside'].sum())}")
    if n >= 64:
        assert 1 <= dev_flags.sum() < n, (tag, int(dev_flags.sum()))
    # the weights from the device's own inputs
    assert np.allclose(views["ratio"][~band], np.fmin(u, cap)[~band], rtol=1e-15, atol=0.0), tag
    assert np.all(views["ratio"][dev_flags == 1] == cap) and np.all(views["ratio"] <= cap), tag
    # gradients per tensor, and the per-sample log-probabilities
    rel = {}
    if n < 32:
        hb32 = _host(c["env"].handle.onpolicy_batch(5, step, 0, 32))
        assert hb32["indices"][0] == idx[0]
        a32 = c["actions"][hb32["indices"]]
        rel = _single_rows(lambda r, ex: awr_grad_np(layers, hb32["observations"][r], a32[r], hb32["advantages"][r], temperature, cap, ent, exact=ex, **kw))
    gW, gb = learner.gradients("policy")
    for l in range(len(layers)):
        _within(tag, f"policy dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
        _within(tag, f"policy db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"))
    _within(tag, "log_probs_new", views["log_probs_new"], exact["log_probs_new"], f32["log_probs_new"], rel.get("log_probs_new"))
    # statistics against fsum over the device's own arrays
    st = learner.stats("policy")
    terms = views["ratio"] * views["log_probs_new"]
    assert np.array_equal(views["loss_terms"], terms), tag
    surr, entropy = math.fsum(terms) / n, math.fsum(views["entropy_terms"]) / n
    b_surr, b_ent = _mean_bound(terms, n), _mean_bound(views["entropy_terms"], n)
    assert abs(st["surrogate"] - surr) <= b_surr and abs(st["entropy"] - entropy) <= b_ent, (tag, st, surr, entropy)
    assert abs(st["loss"] - (-surr - ent * entropy)) <= b_surr + abs(ent) * b_ent + 4 * U * (abs(surr) + abs(ent) * abs(entropy)), (tag, st)
    assert st["clip_fraction"] == int(dev_flags.sum()) / n and math.isnan(st["value_loss"]), (tag, st)
    if lp_old is None:
        assert math.isnan(st["approx_kl"]), (tag, st)
    else:
        kl_terms = lp_old - views["log_probs_new"]
        assert abs(st["approx_kl"] - math.fsum(kl_terms) / n) <= _mean_bound(kl_terms, n), (tag, st)
    _grad_norm_ok(tag, learner, "policy", st)
    return exact


def _check_expectile_step(tag, c, learner, net, hb, params, n, step, tau):
    ret = hb["returns"] if net == "value" else hb["cost_returns"][CHANNELS[net]]
    layers = _pairs(*params)
    kw = dict(activation=c["activation"])
    exact = expectile_grad_np(layers, hb["observations"], ret, tau, exact=True, **kw)
    f32 = expectile_grad_np(layers, hb["observations"], ret, tau, exact=False, **kw)
    rel = {}
    if n < 32:
        hb32 = _host(c["env"].handle.onpolicy_batch(5, step, 0, 32))
        r32 = hb32["returns"] if net == "value" else hb32["cost_returns"][CHANNELS[net]]
        rel = _single_rows(lambda r, ex: expectile_grad_np(layers, hb32["observations"][r], r32[r], tau, exact=ex, **kw))
    gW, gb = learner.gradients(net)
    d = exact["values"] - ret.astype(np.float64)
    q = np.where(d < 0.0, tau, 1.0 - tau)
    for l in range(len(layers)):
        _within(tag, f"{net} dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
        floor = 2.0 ** -24 * math.fsum(np.abs(q * (2.0 * d) / n)) if l == len(layers) - 1 else None
        _within(tag, f"{net} db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"), floor)
    views = learner.views(net)
    assert views["log_probs_new"] is None and views["ratio"] is None and views["clipped"] is None
    terms = views["loss_terms"].to_host()
    st = learner.stats(net)
    assert abs(st["value_loss"] - math.fsum(terms) / n) <= _mean_bound(terms, n) and st["loss"] == st["value_loss"], (tag, st)
    assert all(math.isnan(st[k]) for k in ("surrogate", "entropy", "approx_kl", "clip_fraction"))
    _grad_norm_ok(tag, learner, net, st)
    return exact


def _temperature(c, adv_norm):
    return 1.0 if adv_norm == "rollout" else c["adv_std"]


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


ALL = [("ieee13-relu", n, adv) for n in (1, 64, 65, 185) for adv in ("none", "rollout")] + [("ieee13-elu", 185, "rollout"), ("ieee123-relu", 65, "rollout"),
                                                                                          ("ieee123-relu", 185, "none")]


@pytest.mark.parametrize("name,n,adv_norm", ALL, ids=[f"{a}-n{b}-{c}" for a, b, c in ALL])
def test_three_offline_steps_against_the_restatements(prepared, name, n, adv_norm):
    """AWR on the policy, the expectile loss (0.7) on the reward critic and on the thermal cost critic, on a random-action rollout:
    gradients, flags, weights, per-sample arrays and statistics at freshly created parameters and after two steps; the cap is set
    anew for every minibatch between the steps (``_cap``), and Adam's parameters and moments follow ``adam_np`` bit for bit over the
    three steps, so ``set_loss`` kept m, v and the step count.

    Observed on the MI355X: see DESIGN.md section 21 "Observed accuracy"."""
    c = prepared(name)
    h = c["env"].handle
    if name == "ieee123-relu":
        assert c["env"].action_dim == 8
    _install(c)
    c["batches"][adv_norm].prepare()
    MISSED.clear()
    learner = P.DeviceLearner(c["env"], nets=NETS, **HYPER, **OFFLINE)
    assert learner.loss("policy")["name"] == "awr" and learner.loss("value")["name"] == "expectile" and learner.loss("thermal")["expectile"] == TAU
    temperature = _temperature(c, adv_norm)
    state = {net: learner.download(net) for net in NETS}
    seen_outside, below = 0, 0
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = _host(batch)
        cap = _cap(hb["advantages"], temperature)
        learner.set_loss("policy", "awr", temperature=temperature, weight_max=cap)
        assert learner.loss("policy") == dict(kind="awr", name="awr", temperature=temperature, weight_max=cap, expectile=0.0)
        params = {net: learner.parameters(net) for net in NETS}
        learner.step(batch)
        if s in (0, 2):
            tag = f"{name} n={n} {adv_norm} step {s + 1}"
            ex = _check_awr_step(tag, c, learner, hb, params["policy"], n, s, temperature, cap)
            seen_outside += int(ex["log_std_outside"].sum())
            for net in ("value", "thermal"):
                ev = _check_expectile_step(tag, c, learner, net, hb, params[net], n, s, TAU)
                if net == "value" and n >= 64:
                    assert 1 <= ev["below"].sum() < n, (tag, int(ev["below"].sum()))          # both signs of v - ret
                    below += 1
        for net in NETS:
            g = learner.download(net, ("grads",))["grads"]
            st = learner.stats(net)
            assert st["step"] == s + 1
            p, m, v = adam_np(state[net]["params"], g, state[net]["m"], state[net]["v"], s + 1, HYPER, st["grad_norm"])
            got = learner.download(net)
            assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v), (name, n, net, s)
            state[net] = got
    if CASES[name][3]:
        assert seen_outside >= 1
    assert not MISSED, MISSED


@pytest.mark.parametrize("tau", [0.1, 0.7])
def test_expectile_gradients_at_both_expectiles(prepared, tau):
    c = prepared("ieee13-relu")
    h = c["env"].handle
    _install(c)
    c["batches"]["rollout"].prepare()
    MISSED.clear()
    learner = P.DeviceLearner(c["env"], nets=("value", "thermal"), **HYPER, value_loss="expectile", expectile=tau)
    for s in range(2):
        batch = h.onpolicy_batch(5, s, 0, 185)
        hb = _host(batch)
        params = {net: learner.parameters(net) for net in learner.nets}
        learner.step(batch)
        for net in learner.nets:
            ev = _check_expectile_step(f"tau={tau} step {s + 1}", c, learner, net, hb, params[net], 185, s, tau)
            if net == "value":
                assert 1 <= ev["below"].sum() < 185
    assert not MISSED, MISSED


def test_expectile_at_one_half_is_half_of_a_mean_squared_error_twin_bit_for_bit(prepared):
    c = prepared("ieee13-relu")
    h = c["env"].handle
    c["batches"]["rollout"].prepare()
    out = []
    for kw in (dict(), dict(value_loss="expectile", expectile=0.5)):
        _install(c)
        learner = P.DeviceLearner(c["env"], nets=("value", "thermal"), **HYPER, **kw)
        learner.step(h.onpolicy_batch(5, 0, 0, 185))
        out.append({net: (learner.download(net, ("grads",))["grads"], learner.stats(net)["value_loss"], learner.views(net)["loss_terms"].to_host())
                    for net in learner.nets})
    for net in ("value", "thermal"):
        (g_mse, l_mse, t_mse), (g_half, l_half, t_half) = out[0][net], out[1][net]
        assert g_mse.any() and np.array_equal(g_half.view(np.uint32), (np.float32(0.5) * g_mse).view(np.uint32)), net
        assert l_half == 0.5 * l_mse and np.array_equal(t_half, 0.5 * t_mse), net


def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_a_random_action_rollout_trains_the_policy_without_log_probabilities(prepared):
    c = prepared("ieee13-relu")
    h = c["env"].handle
    _install(c)
    c["batches"]["rollout"].prepare()
    learner = P.DeviceLearner(c["env"], nets=("policy",), **HYPER)
    batch = h.onpolicy_batch(5, 0, 0, 185)
    before = learner.download("policy")
    _refused(lambda: learner.step(batch), S, "the last rollout recorded no log-probabilities (a stochastic GS_POLICY_MLP rollout does)")
    assert _same_state(before, learner.download("policy")) and learner.info("policy")["step"] == 0
    learner.set_loss("policy", "awr", temperature=1.0, weight_max=20.0)
    learner.step(batch)
    st = learner.stats("policy")
    assert st["step"] == 1 and math.isnan(st["approx_kl"]) and math.isfinite(st["loss"]) and st["grad_norm"] > 0.0
    learner.set_loss("policy", "ppo")
    _refused(lambda: learner.step(batch), S, "recorded no log-probabilities")


def test_on_a_stochastic_rollout_approx_kl_is_the_mean_of_the_log_probability_differences(prepared):
    c = prepared("ieee13-relu", "policy")
    h = c["env"].handle
    _install(c)
    c["batches"]["rollout"].prepare()
    MISSED.clear()
    learner = P.DeviceLearner(c["env"], nets=("policy",), **HYPER, policy_loss="awr")
    for s in range(2):
        batch = h.onpolicy_batch(5, s, 0, 185)
        hb = _host(batch)
        cap = _cap(hb["advantages"], 1.0)
        learner.set_loss("policy", "awr", temperature=1.0, weight_max=cap)
        params = learner.parameters("policy")
        learner.step(batch)
        _check_awr_step(f"stochastic step {s + 1}", c, learner, hb, params, 185, s, 1.0, cap)          # (approx_kl against fsum inside)
        kl = learner.stats("policy")["approx_kl"]
        assert math.isfinite(kl) and (s == 0 or kl != 0.0)
    assert not MISSED, MISSED


def test_uploaded_actions_at_exactly_plus_and_minus_one_give_finite_gradients():
    env = _env("ieee13")
    rng = np.random.default_rng(4)
    actions = rng.uniform(-1.0, 1.0, (T, B, env.action_dim))
    actions[::3, :, 0] = 1.0
    actions[1::3, :, -1] = -1.0
    actions[5] = 1.0
    actions[6] = -1.0
    env.close()
    c = _build("ieee13-relu", actions)
    try:
        assert np.array_equal(c["actions"], actions.reshape(B * T, -1)) and (np.abs(c["actions"]) == 1.0).sum() >= 2 * B
        h = c["env"].handle
        MISSED.clear()
        learner = P.DeviceLearner(c["env"], nets=("policy",), **HYPER, policy_loss="bc")
        assert learner.loss("policy") == dict(kind="awr", name="bc", temperature=INF, weight_max=INF, expectile=0.0)
        batch = h.onpolicy_batch(5, 0, 0, 185)
        hb = _host(batch)
        params = learner.parameters("policy")
        learner.step(batch)
        views = {k: v.to_host() for k, v in learner.views("policy").items()}
        assert np.all(views["ratio"] == 1.0) and not views["clipped"].any() and np.array_equal(views["loss_terms"], views["log_probs_new"])
        got = learner.download("policy")
        assert all(np.all(np.isfinite(got[k])) for k in got) and got["grads"].any() and np.all(np.isfinite(views["log_probs_new"]))
        layers = _pairs(*params)
        act = c["actions"][hb["indices"]]
        exact = awr_grad_np(layers, hb["observations"], act, hb["advantages"], INF, INF, ENT, exact=True)
        f32 = awr_grad_np(layers, hb["observations"], act, hb["advantages"], INF, INF, ENT, exact=False)
        gW, gb = learner.gradients("policy")
        for l in range(len(layers)):
            _within("saturated", f"policy dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0])
            _within("saturated", f"policy db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1])
        assert not MISSED, MISSED
    finally:
        c["env"].close()


def _three_steps(c, n=185, nets=NETS, **kw):
    _install(c)
    c["batches"]["rollout"].prepare()
    learner = P.DeviceLearner(c["env"], nets=nets, **HYPER, **kw)
    for s in range(3):
        learner.step(c["env"].handle.onpolicy_batch(5, s, 0, n))
    return learner


def test_two_twins_end_with_the_same_bits(prepared):
    c = prepared("ieee13-relu")
    other = _build("ieee13-relu")
    a, b = _three_steps(c, **OFFLINE), _three_steps(other, **OFFLINE)
    for net in NETS:
        assert _same_state(a.download(net), b.download(net)), net
        assert all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a.stats(net).values(), b.stats(net).values())), net
    other["env"].close()


def test_lifetime_rules_and_nothing_changes_on_refusal(prepared):
    c = prepared("ieee13-relu")
    env, h = c["env"], c["env"].handle
    reference = {net: _three_steps(c, **OFFLINE).download(net) for net in ("policy", "value")}          # what three valid steps give
    default = dict(kind="default", temperature=0.0, weight_max=0.0, expectile=0.0)
    _install(c)
    _refused(lambda: h.learner_get_loss("policy"), S, "no learner")
    _refused(lambda: h.learner_set_loss("policy", _lib.learner_loss("awr")), S, "no learner")
    learner = P.DeviceLearner(env, nets=NETS, **HYPER)
    assert all(h.learner_get_loss(net) == default for net in NETS)
    # round trips
    for net, kw in (("policy", dict(kind="awr", temperature=0.25, weight_max=INF, expectile=0.9)), ("policy", dict(kind="awr", temperature=INF, weight_max=3.0, expectile=0.0)),
                    ("value", dict(kind="expectile", temperature=-4.0, weight_max=0.0, expectile=0.3)), ("thermal", dict(kind="expectile", temperature=1.0, weight_max=1.0, expectile=0.99)),
                    ("value", dict(kind="default", temperature=INF, weight_max=-1.0, expectile=7.0))):          # (fields the kind does not use are ignored, and kept)
        h.learner_set_loss(net, _lib.learner_loss(**kw))
        assert h.learner_get_loss(net) == kw, (net, kw)
    # gs_learner_create resets the loss; a *_set* entry ends it with the learner, and only that learner's
    learner = P.DeviceLearner(env, nets=NETS, **HYPER)
    assert all(h.learner_get_loss(net) == default for net in NETS)
    learner.set_loss("policy", "awr", temperature=1.0, weight_max=20.0)
    learner.set_loss("value", "expectile", expectile=TAU)
    learner.set_loss("thermal", "expectile", expectile=TAU)
    env.set_value(c["vals"]["value"])
    _refused(lambda: h.learner_get_loss("value"), S, "no learner")
    assert learner.loss("policy")["name"] == "awr" and learner.loss("thermal")["name"] == "expectile"
    h.learner_create("value", _lib.learner_config(**HYPER))
    assert h.learner_get_loss("value") == default
    learner.set_loss("value", "expectile", expectile=TAU)
    want = {net: h.learner_get_loss(net) for net in NETS}
    # every rule of gs_learner_set_loss
    nan = float("nan")
    loss = _lib.learner_loss
    refusals = [
        (lambda: h.learner_set_loss("policy", loss("awr", struct_size=24)), I, "struct_size"),
        (lambda: h.learner_set_loss("policy", loss(3)), I, "unknown kind"),
        (lambda: h.learner_set_loss("value", loss(-1)), I, "unknown kind"),
        (lambda: h.learner_set_loss("value", loss("awr")), I, "GS_LOSS_AWR"),
        (lambda: h.learner_set_loss("thermal", loss("awr")), I, "GS_LOSS_AWR"),
        (lambda: h.learner_set_loss("policy", loss("expectile")), I, "GS_LOSS_EXPECTILE"),
        (lambda: h.learner_set_loss("policy", loss("awr", temperature=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("policy", loss("awr", weight_max=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("policy", loss("awr", expectile=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("policy", loss("default", temperature=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("value", loss("expectile", expectile=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("value", loss("expectile", weight_max=nan)), I, "NaN"),
        (lambda: h.learner_set_loss("policy", loss("awr", temperature=0.0)), I, "temperature > 0"),
        (lambda: h.learner_set_loss("policy", loss("awr", temperature=-1.0)), I, "temperature > 0"),
        (lambda: h.learner_set_loss("policy", loss("awr", temperature=-INF)), I, "temperature > 0"),
        (lambda: h.learner_set_loss("policy", loss("awr", weight_max=0.0)), I, "weight_max > 0"),
        (lambda: h.learner_set_loss("policy", loss("awr", weight_max=-INF)), I, "weight_max > 0"),
        (lambda: h.learner_set_loss("value", loss("expectile", expectile=0.0)), I, "0 < expectile < 1"),
        (lambda: h.learner_set_loss("value", loss("expectile", expectile=1.0)), I, "0 < expectile < 1"),
        (lambda: h.learner_set_loss("thermal", loss("expectile", expectile=INF)), I, "0 < expectile < 1"),
        (lambda: h._check(h._lib.gs_learner_set_loss(h._h, 7, ctypes.byref(loss("awr")))), I, "unknown net"),
        (lambda: h._check(h._lib.gs_learner_get_loss(h._h, -1, ctypes.byref(loss("awr")))), I, "unknown net"),
        (lambda: h._check(h._lib.gs_learner_set_loss(h._h, 0, None)), I, "NULL"),
        (lambda: h.learner_set_loss("voltage", loss("expectile")), S, "no learner"),
        (lambda: h.learner_get_loss("voltage"), S, "no learner"),
    ]
    for call, code, text in refusals:
        _refused(call, code, text)
    assert {net: h.learner_get_loss(net) for net in NETS} == want
    # nothing changed by any of them: the same three valid steps give the bits they gave before
    _install(c)
    learner = P.DeviceLearner(env, nets=NETS, **HYPER, **OFFLINE)
    for s in range(3):
        for call, code, text in refusals[s::3]:
            _refused(call, code, text)
        learner.step(h.onpolicy_batch(5, s, 0, 185))
    for net in reference:
        assert _same_state(learner.download(net), reference[net]), net
    # set_loss between steps keeps m, v and the step count: the next step is adam_np from the kept state
    kept = learner.download("policy")
    learner.set_loss("policy", "bc")
    assert _same_state(learner.download("policy", ("params", "m", "v")), {k: kept[k] for k in ("params", "m", "v")}) and learner.info("policy")["step"] == 3
    learner.step(h.onpolicy_batch(5, 3, 0, 185))
    got, st = learner.download("policy"), learner.stats("policy")
    assert st["step"] == 4 and st["clip_fraction"] == 0.0
    p, m, v = adam_np(kept["params"], got["grads"], kept["m"], kept["v"], 4, HYPER, st["grad_norm"])
    assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v)


def test_a_learner_left_at_the_defaults_behaves_as_before(prepared):
    """the clipped surrogate and a mean-squared-error cost critic on a handle whose reward critic was moved to the expectile loss and
    whose losses are read, against a twin handle that never calls the new entries: the same bits over three steps"""
    c = prepared("ieee13-relu", "policy")
    twin = _build("ieee13-relu", "policy")
    out = []
    for k, x in enumerate((c, twin)):
        _install(x)
        x["batches"]["rollout"].prepare()
        learner = P.DeviceLearner(x["env"], nets=NETS, **HYPER)
        if k == 0:
            assert learner.loss("policy")["name"] == "ppo" and learner.loss("thermal")["name"] == "mse"
            learner.set_loss("value", "expectile", expectile=TAU)
        per_step = []
        for s in range(3):
            learner.step(x["env"].handle.onpolicy_batch(5, s, 0, 185))
            if k == 0:
                learner.loss("policy")
            per_step.append({net: learner.download(net) for net in ("policy", "thermal")})
        out.append(per_step)
        st = learner.stats("policy")
        assert math.isfinite(st["approx_kl"]) and st["step"] == 3
    for s in range(3):
        for net in ("policy", "thermal"):
            assert _same_state(out[0][s][net], out[1][s][net]), (s, net)
    assert out[0][2]["policy"]["params"].any() and not np.array_equal(out[0][2]["policy"]["params"], out[0][0]["policy"]["params"])
    twin["env"].close()
    _PREPARED.pop(("ieee13-relu", "policy"))["env"].close()


def test_a_federated_round_over_two_awr_clients_keeps_their_losses(prepared):
    c = prepared("ieee13-relu")
    other = _build("ieee13-relu")
    fed = None
    try:
        kw = dict(policy_loss="awr", temperature=0.5, weight_max=7.0, value_loss="expectile", expectile=0.6)
        learners = []
        for x in (c, other):
            _install(x)
            x["batches"]["rollout"].prepare()
            learners.append(P.DeviceLearner(x["env"], nets=("policy", "value"), **HYPER, **kw))
        fed = P.FederatedLearners(learners)
        for k, (x, l) in enumerate(zip((c, other), learners)):
            for s in range(1 + k):                                  # (different numbers of local steps: different parameters)
                l.step(x["env"].handle.onpolicy_batch(5, s, 0, 64 + k))
        want = [{net: l.loss(net) for net in l.nets} for l in learners]
        assert want[0]["policy"]["name"] == "awr" and want[0]["policy"]["weight_max"] == 7.0 and want[1]["value"]["expectile"] == 0.6
        g0 = {net: fed.global_parameters(net) for net in ("policy", "value")}
        kept = {net: [l.download(net) for l in learners] for net in ("policy", "value")}
        out = fed.round(weights=[40.0, 25.0], clip_norm=0.02)
        for net in ("policy", "value"):
            assert not np.array_equal(kept[net][0]["params"], kept[net][1]["params"])
            agg = fedavg_np(g0[net], [kept[net][k]["params"] for k in range(2)], [40.0, 25.0], norms=out[net]["norms"], clip_norm=0.02)
            for l in learners:
                assert np.array_equal(l.download(net, ("params",))["params"].view(np.uint32), agg.view(np.uint32)), net
        assert [{net: l.loss(net) for net in l.nets} for l in learners] == want
        # and the clients go on with their own losses: the next step is an AWR step from the aggregated parameters
        for k, (x, l) in enumerate(zip((c, other), learners)):
            before = l.download("policy")
            l.step(x["env"].handle.onpolicy_batch(5, 2, 0, 64))
            got, st = l.download("policy"), l.stats("policy")
            assert st["step"] == 2 + k and math.isnan(st["approx_kl"])
            p, m, v = adam_np(before["params"], got["grads"], before["m"], before["v"], 2 + k, HYPER, st["grad_norm"])
            assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v)
    finally:
        if fed is not None:
            fed.close()
        other["env"].close()
