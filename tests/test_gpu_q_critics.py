"""GPU: state-action critics (include/gridstep.h "state-action critics") -- the twin Q networks over a rollout's
stored (observation, action) pairs, the TD target, the Q learner, the target networks and the Q-based signals of the policy's and the
reward critic's heads, against the NumPy restatements of grid_fed_rl_gym_amd (``q_rollout_np``, ``q_combine_np``, ``td_target_np``,
``polyak_np``, ``value_grad_np``, ``adam_np``, ``fedavg_np``).

The dataset is what an offline client holds: a RANDOM-ACTION rollout.  13-bus: T = 37 steps of B = 5 instances (N = 185 rows: two full
64-row tiles and one of 57), obs_dim 71 and action_dim 3 -- the boundary between the two sources falls inside a lane's pair of
columns --, ``episode_length`` 14 under voltage limits (0.98, 1.02): some episodes end at the time limit (bit 0) and some after more
than ten violating steps (bit 1); both are asserted.  123-bus: T = 3, B = 70, hidden 256, 256; 692 input columns are 44 blocks in
three panels, and B is no multiple of the tile.  An 11-bus synthetic feeder (obs_dim 113, action_dim 4: 117 columns) puts the boundary
to the padding inside a lane's pair as well; T = 9, B = 9 (81 rows).

Bounds, none of them computed from the device:
  q, gradients     within 4 E_ref, E_ref = the float32 restatement's own error against ``exact=True`` on the same rows (section 15's
                   rule; for the learner section 19's, with its two amendments: below 32 rows E_ref from 32 single rows relative to the
                   tensor's largest entry, and for a one-entry tensor at least the float32 rounding of the terms)
  everything else  bit-equal: q_min, q_adv and td_target to the restatements fed the device's own q, values and terminal values; online
                   and target images after install; rows under another B; Adam; the target update; the signals (the same head kernels
                   on equal inputs); twins; the federated round."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.federated import fedavg_np
from grid_fed_rl_gym_amd.learner import adam_np, awr_grad_np, expectile_grad_np, value_grad_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, polyak_np, q_combine_np, q_rollout_np, rollout_device, td_target_np

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like, "scal11": lambda: P.scalable_like(11, seed=1)}
SOLVER = {"scal11": "nr"}       # (a feeder with loops)
# name: (feeder, B, T, episode_length, hidden widths, activation)
CASES = {
    "ieee13-relu": ("ieee13", 5, 37, 14, [64, 64], "relu"),
    "ieee13-tanh40": ("ieee13", 5, 37, 14, [40, 40], "tanh"),
    "ieee13-elu": ("ieee13", 5, 37, 14, [64, 64], "elu"),
    "ieee123-relu": ("ieee123", 70, 3, 2, [256, 256], "relu"),
    "ieee13-single": ("ieee13", 5, 37, 14, [], "relu"),
    "scal11-relu": ("scal11", 9, 9, 3, [64, 64], "relu"),
}
GAMMA = 0.97
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, clip=0.2, ent_coef=0.01, max_grad_norm=0.5)
FIELDS = ["observations", "actions", "advantages", "returns", "values", "indices"]
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
WORST = {}
MISSED = []


def _env(feeder, num_envs, episode_length):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=num_envs, solver=SOLVER.get(feeder, "fbs"), stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=episode_length, voltage_limits=(0.98, 1.02))


_NORM = {}


def _normalisation(feeder):
    if feeder not in _NORM:
        env = _env(feeder, 64, 7)
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


def _networks(feeder, D, A, hidden, activation):
    mean, std = _normalisation(feeder)
    pol = P.MLPPolicy(*_layers([D, 64, 2 * A], 1), activation="relu", head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    val = P.MLPValue(*_layers([D, 64, 1], 2), activation="relu", obs_mean=mean, obs_std=std)
    qs = [P.MLPQ(*_layers([D + A] + hidden + [1], 20 + w), D, activation=activation, obs_mean=mean, obs_std=std) for w in range(2)]
    return pol, val, qs


def _shifted(val, shift):
    bs = [b.copy() for b in val.biases]
    bs[-1][0] += shift
    return P.MLPValue(val.weights, bs, activation=val.activation, obs_mean=val.obs_mean, obs_std=val.obs_std)


def _install(c, qs=None, twins=(0, 1)):
    """the networks as first installed: ends every learner of the handle"""
    env = c["env"]
    env.set_policy(c["pol"], stochastic=True)
    env.set_value(c["val"])
    for w in twins:
        env.set_q(w, (qs or c["qs"])[w])


def _evaluate(env, mask=3):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=mask)
    return P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=mask)


def _rollout_arrays(env):
    h = env.handle
    d = h.rollout_download(want=("observations", "actions", "rewards", "terminals"))
    dev = h.rollout_device_arrays()
    d["terminal_index"] = dev["terminal_index"].to_host()
    return d


def _build(name):
    feeder, B, T, ep, hidden, activation = CASES[name]
    env = _env(feeder, B, ep)
    pol, val, qs = _networks(feeder, env.obs_dim, env.action_dim, hidden, activation)
    c = dict(env=env, pol=pol, val=val, qs=qs, feeder=feeder, activation=activation, B=B, T=T, ep=ep, name=name)
    _install(c)
    env.reset(seed=3)
    rollout_device(env, T, seed=7, reset=False)
    c["data"] = _rollout_arrays(env)
    _evaluate(env)
    # V moved so that v - min(Q1, Q2) has both signs
    got = env.handle.rollout_q_download(("q_min",))["q_min"]["target"]
    v = env.handle.rollout_onpolicy_download(("values",))["values"]
    c["val"] = _shifted(val, float(np.median(got - v[:T])))
    env.set_value(c["val"])
    _evaluate(env)
    c["batches"] = OnPolicyBatches(env, B * T, policy=pol, adv_norm="none", seed=5, fields=FIELDS)
    c["batches"].prepare()
    return c


_PREPARED = {}


@pytest.fixture(scope="module")
def prepared():
    def get(name):
        if name not in _PREPARED:
            _PREPARED[name] = _build(name)
        return _PREPARED[name]
    yield get
    for c in _PREPARED.values():
        c["env"].close()
    _PREPARED.clear()
    print("largest device error / E_ref:", {k: round(v, 3) for k, v in WORST.items()})


def _twin(c, qs, B=None, twins=(0, 1)):
    """another handle with ``qs`` installed as the Q networks, on which the rollout of ``c`` is repeated (the first ``B`` instances,
    their stored actions uploaded); returns (env, its rollout's arrays)"""
    B = B or c["B"]
    env = _env(c["feeder"], B, c["ep"])
    t = dict(c, env=env)
    _install(t, qs, twins)
    env.reset(seed=3)
    nb = min(B, c["B"])
    act = np.zeros((c["T"], B, env.action_dim))
    act[:, :nb] = c["data"]["actions"][:, :nb]
    if B > nb:
        act[:, nb:] = np.random.default_rng(9).uniform(-1.0, 1.0, act[:, nb:].shape)
    rollout_device(env, c["T"], reset=False, actions=act)
    return env, _rollout_arrays(env)


def _host(batch):
    return {k: v.to_host() for k, v in batch.items() if v is not None and not isinstance(v, list)}


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


def _within(tag, what, got, exact, f32, rel_ref=None, floor=None):
    """section 19's bound with its two amendments (tests/test_gpu_learner.py ``_within``)"""
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    if rel_ref is not None:
        e_ref = rel_ref * float(np.max(np.abs(exact)))
    if floor is not None:
        e_ref = max(e_ref, floor)
    ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    key = what.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio if math.isfinite(ratio) else 1e9)
    if not e_dev <= 4.0 * e_ref:          # (every tensor of the step is looked at before the test fails)
        MISSED.append((tag, what, e_dev, e_ref))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def _to_device(dev, host):
    """overwrites the device array ``dev`` (a view of a minibatch field) with ``host``, of the same shape and dtype"""
    host = np.ascontiguousarray(host, dtype=np.dtype(dev.typestr))
    assert host.shape == dev.shape
    rc = _lib._hip_runtime().hipMemcpy(ctypes.c_void_p(dev.ptr), ctypes.c_void_p(host.ctypes.data), ctypes.c_size_t(host.nbytes), 1)      # hipMemcpyHostToDevice
    assert rc == 0


# ---- evaluation --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_q_of_every_stored_pair_against_the_restatement(prepared, name):
    """Observed on the MI355X: see DESIGN.md section 22 "Observed accuracy"."""
    c = prepared(name)
    env, d, T, B = c["env"], c["data"], c["T"], c["B"]
    if c["feeder"] == "ieee13":
        assert (env.obs_dim, env.action_dim) == (71, 3)        # obs_dim odd: one lane's pair holds the last observation column and action 0
        flags = d["terminals"]
        assert (flags == 1).any() and ((flags & 2) != 0).any(), "the dataset ends episodes under both done bits"
    elif c["feeder"] == "scal11":
        assert env.obs_dim % 2 == 1 and env.action_dim == 4    # 113 + 4 odd: the last pair holds action 3 and a padded column
        assert (d["terminals"] != 0).any()
    else:
        assert env.obs_dim + env.action_dim == 692 and (d["terminals"] != 0).any()
    _install(c)
    out = _evaluate(env)
    assert out.installed == (0, 1) and out.rows_per_tile == 64 and out.td_target.shape == (T, B)
    got = env.handle.rollout_q_download(("q",))["q"]
    for w in range(2):
        exact = q_rollout_np(c["qs"][w], d["observations"], d["actions"], exact=True)
        e_ref = _err(q_rollout_np(c["qs"][w], d["observations"], d["actions"]), exact)
        err = _err(got["online"][w], exact)
        print(f"{name} twin {w}: E_ref {e_ref:.3e} max |device - exact| {err:.3e} ratio {err / e_ref:.2f}")
        WORST["q"] = max(WORST.get("q", 0.0), err / e_ref)
        assert e_ref > 0.0 and err <= 4.0 * e_ref, (err, e_ref)
        assert np.std(exact) > 1e-3
        assert _same(got["online"][w], got["target"][w]), "the target image is a copy of the online image"
        assert _same(out.q["online"][w].to_host(), got["online"][w])
    assert not np.array_equal(got["online"][0], got["online"][1])
    # one twin alone: the same bits, and the minimum is that twin
    env.set_q(0, None)
    _evaluate(env)
    one = env.handle.rollout_q_download()
    assert np.isnan(one["q"]["online"][0]).all() and _same(one["q"]["online"][1], got["online"][1])
    assert _same(one["q_min"]["online"], got["online"][1]) and _same(one["q_min"]["target"], got["target"][1])
    _install(c)
    _evaluate(env)


@pytest.mark.parametrize("name,B2", [("ieee13-relu", 7), ("ieee13-tanh40", 3), ("ieee123-relu", 37)])
def test_a_rows_q_does_not_depend_on_the_batch_it_lies_in(prepared, name, B2):
    c = prepared(name)
    _install(c)
    _evaluate(c["env"])
    want = c["env"].handle.rollout_q_download(("q",))["q"]
    env, d = _twin(c, c["qs"], B=B2)
    try:
        nb = min(B2, c["B"])
        assert _same(d["observations"][:, :nb], c["data"]["observations"][:, :nb]), "the repeated rollout collects the same observations"
        _evaluate(env)
        got = env.handle.rollout_q_download(("q",))["q"]
        for src in ("online", "target"):
            for w in range(2):
                assert _same(got[src][w][:, :nb], want[src][w][:, :nb]), (src, w)
    finally:
        env.close()


@pytest.mark.parametrize("mask", [0, 1, 3])
def test_minimum_advantage_and_td_target_bit_for_bit(prepared, mask):
    for name in ("ieee13-relu", "ieee123-relu"):
        c = prepared(name)
        env, d = c["env"], c["data"]
        _install(c)
        _evaluate(env, mask)
        got = env.handle.rollout_q_download()
        on = env.handle.rollout_onpolicy_download(("values", "terminal_values"))
        q_on, q_tg, adv = q_combine_np(got["q"]["online"], got["q"]["target"], on["values"])
        assert _same(got["q_min"]["online"], q_on) and _same(got["q_min"]["target"], q_tg) and _same(got["q_adv"], adv), name
        td = td_target_np(d["rewards"], on["values"], d["terminals"], on["terminal_values"], d["terminal_index"], GAMMA, mask)
        assert _same(got["td_target"], td), (name, mask)
        shifted = td_target_np(d["rewards"], on["values"], d["terminals"], on["terminal_values"], d["terminal_index"], GAMMA, mask, 0.5, 0.25)
        env.handle.rollout_evaluate_q(GAMMA, mask, 0.5, 0.25)
        assert _same(env.handle.rollout_q_download(("td_target",))["td_target"], shifted), (name, mask)
        if mask and name == "ieee13-relu":
            ended = d["terminals"] != 0
            assert (td[ended & ((d["terminals"] & mask) != 0)] != (d["rewards"][ended & ((d["terminals"] & mask) != 0)])).any()
        _evaluate(env)


# ---- the Q learner -----------------------------------------------------------------------------------------------------------------

def _single_rows(evaluate):
    worst = {}
    for j in range(32):
        ex, lo = evaluate(slice(j, j + 1), True), evaluate(slice(j, j + 1), False)
        for l, ((ew, eb), (fw, fb)) in enumerate(zip(ex["grads"], lo["grads"])):
            for what, e, f in ((f"dW[{l}]", ew, fw), (f"db[{l}]", eb, fb)):
                top = float(np.max(np.abs(e)))
                if top > 0.0:
                    worst[what] = max(worst.get(what, 0.0), _err(f, e) / top)
    return worst


def _sa(c, hb):
    act = c["data"]["actions"].reshape(c["B"] * c["T"], -1)[hb["indices"]]
    return np.concatenate([hb["observations"], act.astype(np.float32)], axis=1)


STEPS = [("ieee13-relu", n) for n in (1, 33, 64, 65, 185)] + [("ieee13-tanh40", 185), ("ieee13-elu", 65), ("ieee123-relu", 65), ("ieee13-single", 33), ("scal11-relu", 65)]


@pytest.mark.parametrize("name,n", STEPS, ids=[f"{a}-n{b}" for a, b in STEPS])
def test_three_q_steps_against_the_restatements(prepared, name, n):
    """Both twins regress on float32(td_target[idx]) over [obs | float32(act)]: gradients at fresh parameters and after two steps,
    Adam bit for bit over the three steps; then the trained networks evaluate the rollout as a twin handle does on which
    ``learner.q(k)`` was installed (the image, the transposed image and the padding).

    Observed on the MI355X: see DESIGN.md section 22 "Observed accuracy"."""
    c = prepared(name)
    env = c["env"]
    h = env.handle
    _install(c)
    _evaluate(env)
    td = h.rollout_q_download(("td_target",))["td_target"].reshape(-1)
    MISSED.clear()
    nets = ("q1", "q2")
    learner = P.DeviceLearner(env, nets=nets, **HYPER)
    D, A = env.obs_dim, env.action_dim
    for net in nets:
        info = learner.info(net)
        assert info["dims"][0] == D + A and info["dims"][-1] == 1 and learner.loss(net)["name"] == "mse"
    state = {net: learner.download(net) for net in nets}
    kw = dict(activation=c["activation"])
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = _host(batch)
        sa, y = _sa(c, hb), td[hb["indices"]].astype(np.float32)
        params = {net: learner.parameters(net) for net in nets}
        learner.step(batch)
        for net in nets:
            tag = f"{name} n={n} step {s + 1} {net}"
            if s in (0, 2):
                layers = list(zip(*params[net]))
                exact, f32 = value_grad_np(layers, sa, y, exact=True, **kw), value_grad_np(layers, sa, y, exact=False, **kw)
                rel = {}
                if n < 32:
                    hb32 = _host(h.onpolicy_batch(5, s, 0, 32))
                    assert hb32["indices"][0] == hb["indices"][0]
                    sa32, y32 = _sa(c, hb32), td[hb32["indices"]].astype(np.float32)
                    rel = _single_rows(lambda r, ex: value_grad_np(layers, sa32[r], y32[r], exact=ex, **kw))
                gW, gb = learner.gradients(net)
                d = exact["values"] - y.astype(np.float64)
                for l in range(len(layers)):
                    _within(tag, f"dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
                    floor = 2.0 ** -24 * math.fsum(np.abs((2.0 * d) / n)) if l == len(layers) - 1 else None
                    _within(tag, f"db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"), floor)
            g = learner.download(net, ("grads",))["grads"]
            st = learner.stats(net)
            assert st["step"] == s + 1 and st["loss"] == st["value_loss"]
            p, m, v = adam_np(state[net]["params"], g, state[net]["m"], state[net]["v"], s + 1, HYPER, st["grad_norm"])
            got = learner.download(net)
            assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v), (tag,)
            state[net] = got
    assert not MISSED, MISSED
    # the images Adam rewrote, against a fresh install of the same parameters on a twin handle; the targets have not moved
    _evaluate(env)
    got = h.rollout_q_download(("q",))["q"]
    trained = [learner.q(w) for w in range(2)]
    for w in range(2):
        assert _same(learner.target_q(w).weights[0].astype(np.float32), c["qs"][w].weights[0].astype(np.float32))
    twin, d2 = _twin(c, trained)
    try:
        assert _same(d2["observations"], c["data"]["observations"])
        _evaluate(twin)
        want = twin.handle.rollout_q_download(("q",))["q"]
        for w in range(2):
            assert _same(got["online"][w], want["online"][w]), w
            assert not np.array_equal(got["online"][w], got["target"][w])
    finally:
        twin.close()


# ---- target networks ---------------------------------------------------------------------------------------------------------------

def test_target_updates_follow_polyak_np_and_leave_the_online_image_alone(prepared):
    c = prepared("ieee13-tanh40")
    env = c["env"]
    h = env.handle
    _install(c)
    _evaluate(env)
    learner = P.DeviceLearner(env, nets=("q1", "q2"), **HYPER)
    P_count = learner.info("q1")["param_count"]
    # without a step the target equals the online network, and an update whose arithmetic is exact keeps it so
    first = [h.q_target_download(w, P_count) for w in range(2)]
    for w in range(2):
        assert _same(first[w], learner.download(f"q{w + 1}", ("params",))["params"])
    for tau in (1.0, 0.5, 0.0):
        learner.update_targets(tau)
        assert all(_same(h.q_target_download(w, P_count), first[w]) for w in range(2)), tau
    learner.update_targets(0.005)
    assert all(_same(h.q_target_download(w, P_count), polyak_np(first[w], first[w], 0.005)) for w in range(2))
    _install(c)
    _evaluate(env)
    learner = P.DeviceLearner(env, nets=("q1", "q2"), **HYPER)
    for s in range(2):
        learner.step(h.onpolicy_batch(5, s, 0, 185))
    online = [learner.download(f"q{w + 1}", ("params",))["params"] for w in range(2)]
    _evaluate(env)
    before = h.rollout_q_download(("q",))["q"]
    target = first
    for tau in (0.005, 0.5, 1.0):
        learner.update_targets(tau)
        target = [polyak_np(online[w], target[w], tau) for w in range(2)]
        for w in range(2):
            assert _same(h.q_target_download(w, P_count), target[w]), (tau, w)
            assert not np.array_equal(target[w], first[w])
        if tau == 0.5:
            mid = [learner.target_q(w) for w in range(2)]
            _evaluate(env)
            mid_q = h.rollout_q_download(("q",))["q"]
    for w in range(2):
        assert _same(target[w], online[w])                 # tau = 1 copies the online values
        assert _same(learner.download(f"q{w + 1}", ("params",))["params"], online[w])
    _evaluate(env)
    after = h.rollout_q_download(("q",))["q"]
    twin, d2 = _twin(c, mid)
    try:
        assert _same(d2["observations"], c["data"]["observations"])
        _evaluate(twin)
        want = twin.handle.rollout_q_download(("q",))["q"]
        for w in range(2):
            assert _same(after["online"][w], before["online"][w]) and _same(mid_q["online"][w], before["online"][w]), "the online image is untouched"
            assert _same(mid_q["target"][w], want["online"][w]), "the target image is the packed image of the target's parameters"
            assert _same(after["target"][w], after["online"][w])
            assert not np.array_equal(mid_q["target"][w], before["target"][w])
    finally:
        twin.close()


# ---- signals -----------------------------------------------------------------------------------------------------------------------

def _cap(adv, temperature):
    """section 21's weight_max: the geometric midpoint of two adjacent order statistics of exp(A / temperature) near the median that
    lie more than 2e-4 apart relatively"""
    u = np.sort(np.exp(np.asarray(adv).astype(np.float64) / temperature))
    k = len(u) // 2 - 1
    while k + 1 < len(u) and not u[k + 1] > u[k] * (1.0 + 2e-4):
        k += 1
    assert k + 1 < len(u), "no two order statistics above the median lie 2e-4 apart"
    return math.sqrt(float(u[k]) * float(u[k + 1]))


def _step_record(learner, net):
    rec = dict(grads=learner.download(net, ("grads",))["grads"], stats=learner.stats(net))
    rec.update({k: v.to_host() for k, v in learner.views(net).items() if v is not None})
    return rec


def _equal_records(a, b):
    for k in a:
        if k == "stats":
            for s in a[k]:
                x, y = a[k][s], b[k][s]
                assert x == y or (math.isnan(x) and math.isnan(y)), (s, x, y)
        else:
            assert _same(a[k], b[k]), k


@pytest.mark.parametrize("name,n", [("ieee13-relu", 185), ("ieee13-relu", 64), ("ieee123-relu", 65)])
def test_q_signals_are_the_same_heads_on_gathered_inputs(prepared, name, n):
    """lr = 0: every step starts from the same parameters (p - 0 * x = p), so the two paths can run on one learner"""
    c = prepared(name)
    env = c["env"]
    h = env.handle
    _install(c)
    _evaluate(env)
    got = h.rollout_q_download(("q_adv", "q_min"))
    q_adv, q_tgt = got["q_adv"].reshape(-1), got["q_min"]["target"].reshape(-1)
    temperature = float(q_adv.std())
    hyper = dict(HYPER, lr=0.0)
    learner = P.DeviceLearner(env, nets=("policy", "value"), **hyper, policy_loss="awr", temperature=temperature, value_loss="expectile", expectile=0.7)
    assert learner.signal("policy") == "batch" and learner.signal("value") == "batch"
    batch = h.onpolicy_batch(5, 0, 0, n)
    hb = _host(batch)
    idx = hb["indices"]
    adv32, ret32 = q_adv[idx].astype(np.float32), q_tgt[idx].astype(np.float32)
    cap = _cap(adv32, temperature)
    u = np.exp(adv32.astype(np.float64) / temperature)
    assert (np.abs(u - cap) <= 1e-4 * cap).sum() <= 0.02 * n
    learner.set_loss("policy", "awr", temperature=temperature, weight_max=cap)
    params = {net: learner.parameters(net) for net in ("policy", "value")}
    # the Q signals: the batch's advantages and returns are not read (and need not be there)
    learner.set_signal("policy", "q")
    learner.set_signal("value", "q")
    assert learner.signal("policy") == "q" and learner.signal("value") == "q" and learner.loss("policy")["weight_max"] == cap
    learner.step({k: v for k, v in batch.items() if k in ("observations", "indices")})
    by_q = {net: _step_record(learner, net) for net in ("policy", "value")}
    assert all(_same(learner.parameters(net)[0][0], params[net][0][0]) for net in params)
    # the batch signals on the same batch, its buffers overwritten with what the gather reads
    learner.set_signal("policy", "batch")
    learner.set_signal("value", "batch")
    _to_device(batch["advantages"], adv32)
    _to_device(batch["returns"], ret32)
    learner.step(batch)
    by_batch = {net: _step_record(learner, net) for net in ("policy", "value")}
    for net in ("policy", "value"):
        by_q[net]["stats"].pop("step"); by_batch[net]["stats"].pop("step")
        _equal_records(by_q[net], by_batch[net])
        assert by_q[net]["grads"].any()
    # both capped and uncapped samples, both signs of v - q, on the restatements and on the device
    act = c["data"]["actions"].reshape(c["B"] * c["T"], -1)[idx]
    ex = awr_grad_np(list(zip(*params["policy"])), hb["observations"], act, adv32, temperature, cap, HYPER["ent_coef"], exact=True)
    ev = expectile_grad_np(list(zip(*params["value"])), hb["observations"], ret32, 0.7, exact=True)
    flags = by_q["policy"]["clipped"]
    assert np.array_equal(flags, ex["capped"]) and 1 <= flags.sum() < n, int(flags.sum())
    assert 1 <= ev["below"].sum() < n, int(ev["below"].sum())
    assert np.allclose(by_q["policy"]["ratio"], np.fmin(u, cap), rtol=1e-15, atol=0.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_valid_calls_their_bits(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    D, A = env.obs_dim, env.action_dim
    _install(c)
    _evaluate(env)
    want = h.rollout_q_download()
    # the network's rules, on the host alone and at the handle
    good, keep = c["qs"][0].to_struct()
    opts, keep_o = c["qs"][0].to_opts()
    assert _lib.q_check(good, opts, D, A) == (0, "")
    for rc_text, args in (("dims[0] = 74 != obs_dim + action_dim = 75", (good, opts, D, A + 1)), ("action_dim > 0", (good, opts, D + A, 0)),
                          ("GS_COMPUTE_F32", (good, None, D, A))):
        rc, msg = _lib.q_check(*args)
        assert rc == I and rc_text in msg, msg
    wide, keep_w = P.MLPQ(*_layers([D + A, 300, 1], 0), D).to_struct()
    assert _lib.q_check(wide, opts, D, A)[0] == I
    two, keep_t = _lib.policy_struct(*_layers([D + A, 8, 2], 0), "relu", _lib.GS_HEAD_LINEAR, False)
    assert "last width must be 1" in _lib.q_check(two, opts, D, A)[1]
    tanh_head, keep_h = _lib.policy_struct(*_layers([D + A, 8, 1], 0), "relu", "tanh", False)
    assert "GS_HEAD_LINEAR" in _lib.q_check(tanh_head, opts, D, A)[1]
    _refused(lambda: h.set_q(0, wide, opts), I, "outside 1 .. 256")
    _refused(lambda: h._check(h._lib.gs_q_mlp_set(h._h, 2, ctypes.byref(good), ctypes.byref(opts))), I, "which = 2")
    # evaluation
    _refused(lambda: h.rollout_evaluate_q(GAMMA, 4), I, "bootstrap_mask 4")
    _refused(lambda: h.rollout_evaluate_q(math.nan, 3), I, "must be finite")
    _refused(lambda: h.rollout_evaluate_q(GAMMA, 3, struct_size=24), I, "struct_size 24")
    # target networks
    for tau in (-0.1, 1.5, math.nan):
        _refused(lambda: h.q_target_update(tau), I, "outside [0, 1]")
    # signals
    learner = P.DeviceLearner(env, nets=("policy", "value", "q1"), **HYPER, policy_loss="awr")
    _refused(lambda: h.learner_set_signal("q1", "q"), I, "not Q network 0's")
    _refused(lambda: h.learner_set_signal("policy", 2), I, "unknown signal 2")
    _refused(lambda: h.learner_set_signal("voltage", "q"), I, "GS_SIGNAL_Q is the policy's")
    _refused(lambda: h.learner_set_signal("q2", "batch"), S, "no learner for Q network 1")
    _refused(lambda: h.learner_get_signal("q2"), S, "no learner")
    for bad in (7, 9):
        assert h._lib.gs_learner_set_signal(h._h, bad, 0) == I
    _refused(lambda: learner.step({k: v for k, v in h.onpolicy_batch(5, 0, 0, 64).items() if k != "indices"}), I, "the batch lacks indices")
    # the same bits after all of that; the refused network left the installed one in place
    _evaluate(env)
    got = h.rollout_q_download()
    for k in ("q_adv", "td_target"):
        assert _same(got[k], want[k]), k
    for src in ("online", "target"):
        assert _same(got["q_min"][src], want["q_min"][src]) and all(_same(got["q"][src][w], want["q"][src][w]) for w in range(2))
    # what needs a current evaluation refuses before any launch, and a further rollout ends the views
    learner.set_signal("policy", "q")
    batch = h.onpolicy_batch(5, 0, 0, 64)
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)        # (the reward critic's evaluation does not end the Q arrays)
    learner.step(batch)
    kept = {net: learner.download(net) for net in learner.nets}
    env.reset(seed=3)
    rollout_device(env, c["T"], seed=7, reset=False)
    _refused(lambda: h.rollout_q_arrays(), S, "gs_rollout_evaluate_q has not run on the last rollout")
    _refused(lambda: h.rollout_q_download(), S, "gs_rollout_evaluate_q has not run on the last rollout")
    _refused(lambda: h.rollout_evaluate_q(GAMMA, 3), S, "gs_rollout_evaluate has not run on the last rollout")
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    c["batches"].prepare()
    batch = h.onpolicy_batch(5, 0, 0, 64)
    for net in ("policy", "q1"):
        _refused(lambda: h.learner_step(net, batch, 64), S, "gs_rollout_evaluate_q has not run on the last rollout")
    for net in learner.nets:
        now = learner.download(net)
        assert all(_same(now[k], kept[net][k]) for k in now) and learner.info(net)["step"] == 1, net
    h.learner_step("value", batch, 64)                                  # (the batch signal needs no Q evaluation)
    # the same rollout again gives the same arrays
    _install(c)
    _evaluate(env)
    again = h.rollout_q_download()
    assert _same(again["td_target"], want["td_target"]) and _same(again["q_adv"], want["q_adv"])
    c["batches"].prepare()
    # no Q network, no rollout
    env.set_q(0, None)
    env.set_q(1, None)
    _refused(lambda: h.rollout_evaluate_q(GAMMA, 3), S, "before gs_q_mlp_set")
    _refused(lambda: h.q_target_update(0.5), S, "before gs_q_mlp_set")
    _refused(lambda: h.q_target_download(0, 10), S, "not installed")
    _install(c)
    _evaluate(env)
    fresh = _env(c["feeder"], 2, c["ep"])
    try:
        fresh.set_q(0, c["qs"][0])
        _refused(lambda: fresh.handle.rollout_evaluate_q(GAMMA, 3), S, "no rollout has been collected")
    finally:
        fresh.close()


# ---- a whole iteration, non-interference, federation ------------------------------------------------------------------------------------

def _iql_iteration(c, env):
    """V by expectile regression on the target networks' minimum, both twins on the TD target, the policy by AWR on q_adv, the target
    update: two minibatches"""
    _evaluate(env)
    batches = OnPolicyBatches(env, 96, policy=c["pol"], adv_norm="none", seed=5, fields=["observations", "indices"])
    batches.prepare()
    learner = P.DeviceLearner(env, nets=("value", "q1", "q2", "policy"), **HYPER, policy_loss="awr", temperature=3.0, weight_max=20.0, value_loss="expectile",
                              expectile=0.7, advantage_source="q", value_target="q")
    count = 0
    for batch in batches.epoch(0):
        learner.step(batch)
        learner.update_targets(0.3)
        count += 1
    assert count == 2
    out = {net: learner.download(net) for net in learner.nets}
    P_count = learner.info("q1")["param_count"]
    out["targets"] = {w: env.handle.q_target_download(w, P_count) for w in range(2)}
    _evaluate(env)
    out["q"] = env.handle.rollout_q_download()
    return out


def test_two_handles_are_bit_equal_over_an_iql_iteration(prepared):
    c = prepared("ieee13-relu")
    _install(c)
    a = _iql_iteration(c, c["env"])
    twin, d2 = _twin(c, c["qs"])
    try:
        assert _same(d2["observations"], c["data"]["observations"])
        b = _iql_iteration(c, twin)
    finally:
        twin.close()
    for net in ("value", "q1", "q2", "policy"):
        assert all(_same(a[net][k], b[net][k]) for k in a[net]), net
        assert a[net]["grads"].any() and a[net]["m"].any()
    for w in range(2):
        assert _same(a["targets"][w], b["targets"][w]) and not np.array_equal(a["targets"][w], a[f"q{w + 1}"]["params"])
    assert _same(a["q"]["q_adv"], b["q"]["q_adv"]) and _same(a["q"]["td_target"], b["q"]["td_target"])
    assert _same(a["q"]["q_min"]["target"], b["q"]["q_min"]["target"])
    _install(c)
    _evaluate(c["env"])
    c["batches"].prepare()


def test_installed_q_networks_that_are_never_evaluated_change_nothing(prepared):
    c = prepared("ieee13-elu")
    outs = []
    for twins in ((0, 1), ()):
        env = _env(c["feeder"], c["B"], c["ep"])
        try:
            _install(dict(c, env=env), twins=twins)
            env.reset(seed=3)
            rollout_device(env, c["T"], seed=7, reset=False)
            P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
            d = env.handle.rollout_download(want=("observations", "actions", "rewards", "terminals"))
            d.update(env.handle.rollout_onpolicy_download(("values", "terminal_values", "advantages", "returns")))
            outs.append(d)
        finally:
            env.close()
    for k in ("observations", "actions", "rewards", "values", "terminal_values", "advantages", "returns"):
        assert _same(outs[0][k], outs[1][k]), k
    assert np.array_equal(outs[0]["terminals"], outs[1]["terminals"])
    assert _same(outs[0]["observations"], c["data"]["observations"])


def test_a_federated_round_over_two_q_learners_leaves_the_targets_alone(prepared):
    c = prepared("ieee13-relu")
    _install(c)
    _evaluate(c["env"])
    c["batches"].prepare()
    other_env, d2 = _twin(c, c["qs"])
    fed = None
    try:
        _evaluate(other_env)
        OnPolicyBatches(other_env, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS).prepare()
        envs = (c["env"], other_env)
        learners = [P.DeviceLearner(e, nets=("q1", "q2"), **HYPER) for e in envs]
        fed = P.FederatedLearners(learners)
        for k, (e, l) in enumerate(zip(envs, learners)):
            for s in range(1 + k):                                      # (different numbers of local steps: different parameters)
                l.step(e.handle.onpolicy_batch(5, s, 0, 64 + k))
        P_count = learners[0].info("q1")["param_count"]
        targets = [[e.handle.q_target_download(w, P_count) for w in range(2)] for e in envs]
        g0 = {net: fed.global_parameters(net) for net in ("q1", "q2")}
        kept = {net: [l.download(net) for l in learners] for net in ("q1", "q2")}
        out = fed.round(weights=[40.0, 25.0], clip_norm=0.02)
        for w, net in enumerate(("q1", "q2")):
            assert not np.array_equal(kept[net][0]["params"], kept[net][1]["params"])
            agg = fedavg_np(g0[net], [kept[net][k]["params"] for k in range(2)], [40.0, 25.0], norms=out[net]["norms"], clip_norm=0.02)
            for k, (e, l) in enumerate(zip(envs, learners)):
                assert _same(l.download(net, ("params",))["params"], agg), net
                assert _same(e.handle.q_target_download(w, P_count), targets[k][w]), "a round leaves the target images alone"
        # the aggregate reached the online images: both clients evaluate the shared rollout alike, and differently from their targets
        qs = []
        for e in envs:
            _evaluate(e)
            qs.append(e.handle.rollout_q_download(("q",))["q"])
        for w in range(2):
            assert _same(qs[0]["online"][w], qs[1]["online"][w]) and not np.array_equal(qs[0]["online"][w], qs[0]["target"][w])
    finally:
        if fed is not None:
            fed.close()
        other_env.close()
        _install(c)
        _evaluate(c["env"])
