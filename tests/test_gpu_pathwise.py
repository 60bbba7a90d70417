"""GPU: the pathwise actor step (include/gridstep.h "the pathwise actor step") -- the policy's update whose
gradient flows through the twin Q networks -- against the NumPy restatements of grid_fed_rl_gym_amd (``pathwise_grad_np``,
``pathwise_noise_np``, ``adam_np``, ``fedavg_np``).

Feeders and hidden shapes are section 22's: 13-bus, T = 37 steps of B = 5 instances (N = 185 rows), Q input 71 + 3; an 11-bus synthetic
feeder, 113 + 4 columns; 123-bus, T = 3, B = 70, hidden 256, 256 (692 columns).  The hidden widths shape the policy AND the twins.

Bounds, none of them computed from the device:
  noise            within 1e-9 of ``pathwise_noise_np`` (section 12's bound for stochastic actions)
  q, dq_da, dW, db within 4 E_ref of ``exact=True``, E_ref = the float32 restatement's own error on the same rows (section 15's rule; below
                   32 rows E_ref from the 32-row batch that starts with the same rows, relative to the tensor's largest entry: section
                   19's amendment); both restatements are fed the device's noise and take the device's choice of twin
  everything else  bit-equal: the heads to the restatement's heads fed the device's noise, float32 pre-head values, q and dq_da; Adam;
                   the installed image; rows under another n; twins; refusals; non-interference; the federated round."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.federated import fedavg_np
from grid_fed_rl_gym_amd.learner import _pathwise_head, _pathwise_sample, adam_np, pathwise_grad_np, pathwise_noise_np, pathwise_tanh_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, rollout_device

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
ACTOR = dict(alpha=0.2, bc_coef=0.5, pathwise_seed=0x5EED0123456789)
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
    pol = P.MLPPolicy(*_layers([D] + hidden + [2 * A], 1), activation=activation, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    val = P.MLPValue(*_layers([D, 64, 1], 2), activation="relu", obs_mean=mean, obs_std=std)
    qs = [P.MLPQ(*_layers([D + A] + hidden + [1], 20 + w), D, activation=activation, obs_mean=mean, obs_std=std) for w in range(2)]
    return pol, val, qs


def _install(c, qs=None, twins=(0, 1), pol=None):
    """the networks as first installed: ends every learner of the handle"""
    env = c["env"]
    env.set_policy(pol or c["pol"], stochastic=True)
    env.set_value(c["val"])
    for w in range(2):
        env.set_q(w, (qs or c["qs"])[w] if w in twins else None)


def _rollout_arrays(env):
    return env.handle.rollout_download(want=("observations", "actions", "rewards", "terminals"))


def _prepare(c, env):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    b = OnPolicyBatches(env, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS)
    b.prepare()
    return b


def _build(name):
    feeder, B, T, ep, hidden, activation = CASES[name]
    env = _env(feeder, B, ep)
    pol, val, qs = _networks(feeder, env.obs_dim, env.action_dim, hidden, activation)
    c = dict(env=env, pol=pol, val=val, qs=qs, feeder=feeder, activation=activation, B=B, T=T, ep=ep, name=name)
    _install(c)
    env.reset(seed=3)
    rollout_device(env, T, seed=7, reset=False)
    c["data"] = _rollout_arrays(env)
    c["batches"] = _prepare(c, env)
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


def _twin(c, qs=None, twins=(0, 1), pol=None):
    """another handle with the same networks installed, on which the rollout of ``c`` is repeated (its stored actions uploaded) and
    the minibatches prepared; returns a case dict"""
    env = _env(c["feeder"], c["B"], c["ep"])
    t = dict(c, env=env)
    _install(t, qs, twins, pol)
    env.reset(seed=3)
    rollout_device(env, c["T"], reset=False, actions=c["data"]["actions"])
    t["data"] = _rollout_arrays(env)
    assert _same(t["data"]["observations"], c["data"]["observations"]), "the repeated rollout collects the same observations"
    t["batches"] = _prepare(t, env)
    return t


def _learners(env, lr=None, twins=("q1", "q2"), **actor):
    """(the pathwise policy learner, the twins' learners, which no test steps unless it says so)"""
    hyper = HYPER if lr is None else dict(HYPER, lr=lr)
    ql = P.DeviceLearner(env, nets=twins, **hyper) if twins else None
    return P.DeviceLearner(env, nets=("policy",), **hyper, policy_loss="pathwise", **dict(ACTOR, **actor)), ql


def _host(batch):
    return {k: v.to_host() for k, v in batch.items() if v is not None and not isinstance(v, list)}


def _views(learner):
    v = learner.pathwise_views()
    n, A = v["actions"].shape
    out = {k: x.to_host() for k, x in v.items() if hasattr(x, "to_host")}
    flat, stride = out.pop("pre_head"), v["pre_head_stride"]
    out["pre_head"] = np.stack([flat[i * stride:i * stride + 2 * A] for i in range(n)])
    for k in ("q", "dq_da"):
        out[k] = [None if x is None else x.to_host() for x in v[k]]
    out["installed"] = v["installed"]
    return out


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


def _within(tag, what, got, exact, f32, rel_ref=None):
    """section 19's bound with its amendment below 32 rows (tests/test_gpu_learner.py ``_within``)"""
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    if rel_ref is not None:
        e_ref = rel_ref * float(np.max(np.abs(exact)))
    ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    key = what.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio if math.isfinite(ratio) else 1e9)
    if not e_dev <= 4.0 * e_ref:          # (every tensor of the step is looked at before the test fails)
        MISSED.append((tag, what, e_dev, e_ref))
    return e_ref


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _differing(what, got, want):
    """prints how many entries differ and by how many ulps at most, then says whether the two are bit-equal"""
    same = _same(got, want)
    if not same and got.shape == want.shape:
        bad = _bits(got) != _bits(want)
        ulps = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))[bad]
        print(f"{what}: {int(bad.sum())} of {bad.size} entries differ, by at most {int(ulps.max())} ulp")
    return same


def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def _stored(c, hb):
    return c["data"]["actions"].reshape(c["B"] * c["T"], -1)[hb["indices"]]


def _q_layers(ql, nets=("q1", "q2")):
    return [list(zip(*ql.parameters(net))) for net in nets]


def _restate(c, layers, q_layers, hb, noise, exact, which=None, alpha=ACTOR["alpha"], bc_coef=ACTOR["bc_coef"], rows=slice(None)):
    stored = _stored(c, hb)[rows] if bc_coef else None
    return pathwise_grad_np(layers, q_layers, hb["observations"][rows], noise[rows], alpha, bc_coef, stored_actions=stored, exact=exact,
                            which=which, activation=c["activation"], q_activation=c["activation"])


def _record(learner):
    rec = _views(learner)
    rec.update(grads=learner.download("policy", ("grads",))["grads"], stats=learner.stats("policy"))
    return rec


def _equal_records(a, b, skip=("step",)):
    for k in a:
        if k == "stats":
            for s in a[k]:
                x, y = a[k][s], b[k][s]
                assert s in skip or x == y or (math.isnan(x) and math.isnan(y)), (s, x, y)
        elif k in ("q", "dq_da"):
            assert all((x is None and y is None) or _same(x, y) for x, y in zip(a[k], b[k])), k
        elif k == "installed":
            assert a[k] == b[k]
        else:
            assert _same(a[k], b[k]), k


# ---- the step against the restatements (checks 1 to 5) ------------------------------------------------------------------------------

STEPS = [("ieee13-relu", n) for n in (1, 33, 64, 65, 185)] + [("ieee13-tanh40", 185), ("ieee13-elu", 65), ("ieee123-relu", 65), ("ieee13-single", 33), ("scal11-relu", 65)]


@pytest.mark.parametrize("name,n", STEPS, ids=[f"{a}-n{b}" for a, b in STEPS])
def test_three_actor_steps_against_the_restatements(prepared, name, n):
    """Noise, heads, q and dQ/da per twin, the policy's gradient at fresh parameters and after two steps, Adam bit for bit over the
    three steps; then the installed image against a twin handle on which ``learner.policy()`` was installed.

    Observed on the MI355X: see DESIGN.md section 23 "Observed accuracy"."""
    c = prepared(name)
    env = c["env"]
    h = env.handle
    _install(c)
    MISSED.clear()
    learner, ql = _learners(env)
    D, A = env.obs_dim, env.action_dim
    assert learner.loss("policy")["name"] == "pathwise" and learner.info("policy")["dims"][-1] == 2 * A
    q_layers = _q_layers(ql)
    q_state = {net: ql.download(net) for net in ql.nets}
    state = learner.download("policy")
    kw = dict(alpha=ACTOR["alpha"], bc_coef=ACTOR["bc_coef"])
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = _host(batch)
        params = learner.parameters("policy")
        layers = list(zip(*params))
        learner.step(batch)
        v = _views(learner)
        tag = f"{name} n={n} step {s + 1}"
        # 1. the noise, and the heads fed what the device's heads read
        want_noise = pathwise_noise_np(ACTOR["pathwise_seed"], s, n, A)
        e_noise = _err(v["noise"], want_noise)
        print(f"{tag} noise: max |device - pathwise_noise_np| {e_noise:.3e}")
        assert e_noise <= 1e-9 and np.std(v["noise"]) > 0.1
        inside, std, eps, a, lp = _pathwise_sample(v["pre_head"].astype(np.float64), v["noise"])
        heads = [_differing(f"{tag} actions", v["actions"], a), _differing(f"{tag} log_probs", v["log_probs"], lp)]
        found, use, qmin, bc, terms, ghead = _pathwise_head(inside, std, eps, a, lp, v["q"], v["dq_da"], ACTOR["alpha"], ACTOR["bc_coef"], _stored(c, hb), False)
        heads += [_differing(f"{tag} bc_terms", v["bc_terms"], bc), _differing(f"{tag} loss_terms", v["loss_terms"], terms)]
        assert np.array_equal(v["which"], found) and _same(v["q_min"], qmin)
        assert all(heads), tag
        # 2. q and dQ/da per twin, 3. the policy's gradient
        if s in (0, 2):
            rel = {}
            if n < 32:
                hb32 = _host(h.onpolicy_batch(5, s, 0, 32))
                assert hb32["indices"][0] == hb["indices"][0]
                noise32 = pathwise_noise_np(ACTOR["pathwise_seed"], s, 32, A)
                ex32 = _restate(c, layers, q_layers, hb32, noise32, True)
                lo32 = _restate(c, layers, q_layers, hb32, noise32, False, ex32["which"])
                for k in ("q", "dq_da"):
                    rel[k] = _err(lo32[k], ex32[k]) / float(np.max(np.abs(ex32[k])))
                for j in range(32):
                    r = slice(j, j + 1)
                    e1 = _restate(c, layers, q_layers, hb32, noise32, True, rows=r)
                    f1 = _restate(c, layers, q_layers, hb32, noise32, False, e1["which"], rows=r)
                    for l, ((ew, eb), (fw, fb)) in enumerate(zip(e1["grads"], f1["grads"])):
                        for what, e, f in ((f"dW[{l}]", ew, fw), (f"db[{l}]", eb, fb)):
                            top = float(np.max(np.abs(e)))
                            if top > 0.0:
                                rel[what] = max(rel.get(what, 0.0), _err(f, e) / top)
            exact = _restate(c, layers, q_layers, hb, v["noise"], True, v["which"])
            f32 = _restate(c, layers, q_layers, hb, v["noise"], False, v["which"])
            for w in range(2):
                _within(tag, f"q[{w}]", v["q"][w], exact["q"][w], f32["q"][w], rel.get("q"))
                _within(tag, f"dq_da[{w}]", v["dq_da"][w], exact["dq_da"][w], f32["dq_da"][w], rel.get("dq_da"))
            gW, gb = learner.gradients("policy")
            for l in range(len(layers)):
                _within(tag, f"dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
                _within(tag, f"db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"))
            assert np.std(exact["q"]) > 1e-3 and any(np.abs(g).max() > 0.0 for g in gW)
        if not CASES[name][4]:                 # a single-layer Q: the action columns of W0 bit for bit
            for w in range(2):
                w0 = q_layers[w][0][0].astype(np.float32)
                assert _same(v["dq_da"][w], np.ascontiguousarray(np.broadcast_to(w0[0, D:], (n, A)))), w
        # the statistics: what the view holds, reduced
        st = learner.stats("policy")
        assert st["step"] == s + 1 and math.isnan(st["approx_kl"]) and math.isnan(st["clip_fraction"]) and math.isnan(st["value_loss"])
        assert math.isclose(st["loss"], math.fsum(v["loss_terms"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        assert math.isclose(st["surrogate"], math.fsum(v["q_min"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        assert math.isclose(st["entropy"], -math.fsum(v["log_probs"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        # 4. Adam
        g = learner.download("policy", ("grads",))["grads"]
        p, m, vv = adam_np(state["params"], g, state["m"], state["v"], s + 1, HYPER, st["grad_norm"])
        got = learner.download("policy")
        assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], vv), tag
        state = got
    assert not MISSED, MISSED
    # the twins were read, not written
    for net in ql.nets:
        now = ql.download(net)
        assert all(_same(now[k], q_state[net][k]) for k in now) and ql.info(net)["step"] == 0, net
    # 5. the image Adam rewrote, against a fresh install of the same parameters on a twin handle
    trained = learner.policy()
    assert not np.array_equal(trained.weights[0].astype(np.float32), c["pol"].weights[0].astype(np.float32))
    t = _twin(c, pol=trained)
    try:
        for seed, step in ((9, 2), (4, 0)):
            assert _same(env.policy_actions(seed=seed, t=step), t["env"].policy_actions(seed=seed, t=step))
    finally:
        t["env"].close()


@pytest.mark.parametrize("name,n", [("ieee13-relu", 185), ("ieee123-relu", 65)])
def test_the_sampling_head_bit_for_bit(prepared, name, n):
    """``actions`` and ``log_probs`` against ``_pathwise_sample`` fed the device's noise and float32 pre-head values, and the
    deterministic actor's actions against tanh(mean), bit for bit.  The heads' exp, tanh and log are the ones include/gridstep.h
    states operation by operation (``pathwise_exp_np``, ``pathwise_tanh_np``, ``pathwise_log_np`` restate them): a math library's own
    functions agree between device and host to an ulp only -- 136 of 555 actions and 139 of 185 log-probabilities differed on the
    13-bus case when the kernel called them -- and NumPy's differ from build to build.  tanh(mean) is also held to NumPy's within
    4 ulp, what the CPU test holds ``pathwise_tanh_np`` to."""
    c = prepared(name)
    env = c["env"]
    _install(c)
    learner, ql = _learners(env, lr=0.0)
    batch = env.handle.onpolicy_batch(5, 0, 0, n)
    learner.step_pathwise(batch, draw=0)
    v = _views(learner)
    inside, std, eps, a, lp = _pathwise_sample(v["pre_head"].astype(np.float64), v["noise"])
    ok = [_differing(f"{name} actions", v["actions"], a), _differing(f"{name} log_probs", v["log_probs"], lp)]
    learner.step_pathwise(batch, stochastic=False)
    det = _views(learner)
    assert not det["noise"].any() and not np.signbit(det["noise"]).any()
    mean = det["pre_head"][:, :env.action_dim].astype(np.float64)
    ok.append(_differing(f"{name} deterministic actions", det["actions"], pathwise_tanh_np(mean)))
    assert all(ok), ok
    assert np.max(np.abs(_bits(det["actions"]).astype(np.int64) - _bits(np.tanh(mean)).astype(np.int64))) <= 4


# ---- the min's discontinuity (check 6) -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ieee13-relu", "ieee13-tanh40"])
def test_the_smaller_twin_is_the_exact_restatements_away_from_ties(prepared, name):
    c = prepared(name)
    env = c["env"]
    h = env.handle
    n, A = 185, env.action_dim
    _install(c)
    hb = _host(h.onpolicy_batch(5, 0, 0, n))
    noise = pathwise_noise_np(ACTOR["pathwise_seed"], 0, n, A)
    layers = list(zip([c["pol"].weight0] + c["pol"].weights[1:], [c["pol"].bias0] + c["pol"].biases[1:]))      # (as installed: not folded)
    first = _restate(c, layers, [list(zip(q.weights, q.biases)) for q in c["qs"]], hb, noise, True)
    # section 22's construction: twin 1's last bias moved by the median of q_0 - q_1
    bs = [b.copy() for b in c["qs"][1].biases]
    bs[-1][0] += float(np.median(first["q"][0] - first["q"][1]))
    qs = [c["qs"][0], P.MLPQ(c["qs"][1].weights, bs, env.obs_dim, activation=c["activation"], obs_mean=c["qs"][1].obs_mean, obs_std=c["qs"][1].obs_std)]
    q_layers = [list(zip(q.weights, q.biases)) for q in qs]
    exact = _restate(c, layers, q_layers, hb, noise, True)
    f32 = _restate(c, layers, q_layers, hb, noise, False)
    tol = sum(4.0 * _err(f32["q"][w], exact["q"][w]) for w in range(2))
    near = np.abs(exact["q"][0] - exact["q"][1]) <= tol
    # a condition on the inputs: the float32 restatement alone meets what the device is held to
    assert min((exact["which"] == 0).sum(), (exact["which"] == 1).sum()) >= n / 4.0
    assert near.sum() <= 0.05 * n and np.array_equal(f32["which"][~near], exact["which"][~near]), int(near.sum())
    _install(c, qs)
    try:
        learner, ql = _learners(env)
        learner.step(h.onpolicy_batch(5, 0, 0, n))
        v = _views(learner)
        print(f"{name}: twin 0 chosen {(v['which'] == 0).sum()} times, twin 1 {(v['which'] == 1).sum()}; {int(near.sum())} samples within {tol:.3e} of a tie")
        assert min((v["which"] == 0).sum(), (v["which"] == 1).sum()) >= n / 4.0
        assert np.array_equal(v["which"][~near], exact["which"][~near])
        assert _same(v["q_min"], np.where(v["which"] == 0, v["q"][0], v["q"][1]))
    finally:
        _install(c)


# ---- row independence and determinism (checks 7 and 8) -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ieee13-relu", "ieee123-relu"])
def test_a_rows_results_do_not_depend_on_the_batch_it_lies_in(prepared, name):
    c = prepared(name)
    env = c["env"]
    h = env.handle
    _install(c)
    learner, ql = _learners(env, lr=0.0)
    out = []
    for n in (65, 185):
        learner.step_pathwise(h.onpolicy_batch(5, 0, 0, n), draw=3)
        out.append(_views(learner))
    for k in ("actions", "log_probs", "noise"):
        assert _same(out[0][k], out[1][k][:65]), k
    for k in ("q", "dq_da"):
        assert all(_same(out[0][k][w], out[1][k][w][:65]) for w in range(2)), k
    assert _same(out[0]["which"], out[1]["which"][:65]) and not _same(out[0]["loss_terms"], out[1]["loss_terms"][65:130])


def test_determinism_twins_draws_and_the_deterministic_actor(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    _install(c)
    learner, ql = _learners(env, lr=0.0)
    batch = h.onpolicy_batch(5, 0, 0, 185)
    learner.step_pathwise(batch, draw=1)
    a = _record(learner)
    learner.step_pathwise(batch, draw=1)
    _equal_records(a, _record(learner))                        # the same call twice (lr = 0: the same parameters)
    learner.step_pathwise(batch, draw=2)
    other = _record(learner)
    assert not np.array_equal(other["noise"], a["noise"]) and not np.array_equal(other["actions"], a["actions"])
    learner.step_pathwise(batch, draw=1, seed=ACTOR["pathwise_seed"] + 1)
    assert not np.array_equal(_views(learner)["noise"], a["noise"])
    t = _twin(c)
    try:                                                       # two handles
        lt, qt = _learners(t["env"], lr=0.0)
        lt.step_pathwise(t["env"].handle.onpolicy_batch(5, 0, 0, 185), draw=1)
        _equal_records(a, _record(lt), skip=("step",))
    finally:
        t["env"].close()
    learner.step_pathwise(batch, stochastic=False)
    det = _views(learner)
    assert not det["noise"].any() and not np.signbit(det["noise"]).any()
    assert _same(det["actions"], pathwise_tanh_np(det["pre_head"][:, :env.action_dim].astype(np.float64)))
    # one twin alone: the minimum is that twin, with the bits it has beside the other
    for w in range(2):
        _install(c, twins=(w,))
        l1, q1 = _learners(env, lr=0.0, twins=(f"q{w + 1}",))
        l1.step_pathwise(h.onpolicy_batch(5, 0, 0, 185), draw=1)
        v = _views(l1)
        assert v["installed"] == (w,) and v["q"][1 - w] is None and v["dq_da"][1 - w] is None and (v["which"] == w).all()
        assert _same(v["q"][w], a["q"][w]) and _same(v["dq_da"][w], a["dq_da"][w]) and _same(v["q_min"], a["q"][w]) and _same(v["actions"], a["actions"])
    _install(c)


# ---- non-interference (check 9) ---------------------------------------------------------------------------------------------------------

def _q_images(env):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
    return env.handle.rollout_q_download(("q",))["q"]


def test_an_actor_step_leaves_the_twins_alone_and_a_q_step_after_it_is_unchanged(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    _install(c)
    images = _q_images(env)
    learner, ql = _learners(env)
    P_count = ql.info("q1")["param_count"]
    before = {net: ql.download(net) for net in ql.nets}
    targets = [h.q_target_download(w, P_count) for w in range(2)]
    for s in range(2):
        learner.step(h.onpolicy_batch(5, s, 0, 185))
    for w, net in enumerate(ql.nets):
        now = ql.download(net)
        assert all(_same(now[k], before[net][k]) for k in now) and ql.info(net)["step"] == 0, net
        assert _same(h.q_target_download(w, P_count), targets[w])
    after = _q_images(env)
    for src in ("online", "target"):
        assert all(_same(after[src][w], images[src][w]) for w in range(2)), src
    # a Q step after the actor steps, and the same Q step on a twin handle that took none
    ql.step(h.onpolicy_batch(5, 0, 0, 65))
    got = {net: ql.download(net) for net in ql.nets}
    t = _twin(c)
    try:
        _q_images(t["env"])
        qt = P.DeviceLearner(t["env"], nets=("q1", "q2"), **HYPER)
        qt.step(t["env"].handle.onpolicy_batch(5, 0, 0, 65))
        for net in ql.nets:
            want = qt.download(net)
            assert all(_same(got[net][k], want[k]) for k in want) and got[net]["grads"].any(), net
    finally:
        t["env"].close()
    _install(c)


def test_a_handle_that_took_actor_steps_collects_and_learns_as_one_that_took_none(prepared):
    """lr = 0 keeps the parameters' bits (p - 0 x = p) and ``DeviceLearner`` starts Adam afresh, so after the actor steps both handles
    stand where they stood: the same rollout under the policy, the same evaluation, the same critic and advantage-weighted steps."""
    c = prepared("ieee13-elu")
    outs = []
    for actor_steps in (2, 0):
        t = _twin(c)
        env = t["env"]
        try:
            if actor_steps:
                learner, ql = _learners(env, lr=0.0)
                for s in range(actor_steps):
                    learner.step(env.handle.onpolicy_batch(5, s, 0, 185 - s))
            env.reset(seed=21)
            rollout_device(env, 9, seed=13, reset=False, policy=True)
            P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
            d = env.handle.rollout_download(want=("observations", "actions", "rewards"))
            d.update(env.handle.rollout_onpolicy_download(("log_probs", "values", "advantages", "returns")))
            OnPolicyBatches(env, 45, policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS + ["log_probs"]).prepare()
            plain = P.DeviceLearner(env, nets=("policy", "value"), **HYPER)
            plain.step(env.handle.onpolicy_batch(5, 0, 0, 45))
            for net in plain.nets:
                d.update({f"{net}.{k}": x for k, x in plain.download(net).items()})
                d[f"{net}.loss_terms"] = plain.views(net)["loss_terms"].to_host()
            outs.append(d)
        finally:
            env.close()
    for k in outs[0]:
        if isinstance(outs[0][k], np.ndarray):
            assert _same(outs[0][k], outs[1][k]), k
        else:
            assert outs[0][k] == outs[1][k], k
    assert outs[0]["policy.grads"].any() and outs[0]["value.grads"].any()


def test_a_federated_round_over_two_pathwise_policies_is_fedavg_np(prepared):
    c = prepared("ieee13-relu")
    _install(c)
    other = _twin(c)
    fed = None
    try:
        envs = (c["env"], other["env"])
        pairs = [_learners(e) for e in envs]
        learners = [p[0] for p in pairs]
        fed = P.FederatedLearners(learners)
        for k, (e, l) in enumerate(zip(envs, learners)):
            for s in range(1 + k):                                      # (different numbers of local steps: different parameters)
                l.step(e.handle.onpolicy_batch(5, s, 0, 64 + k))
        g0 = fed.global_parameters("policy")
        kept = [l.download("policy") for l in learners]
        assert not np.array_equal(kept[0]["params"], kept[1]["params"])
        out = fed.round(weights=[40.0, 25.0], clip_norm=0.02)
        agg = fedavg_np(g0, [k["params"] for k in kept], [40.0, 25.0], norms=out["policy"]["norms"], clip_norm=0.02)
        for e, l in zip(envs, learners):
            assert _same(l.download("policy", ("params",))["params"], agg)
        # the aggregate reached the installed images: both clients act alike, and a further actor step runs on it
        assert _same(envs[0].policy_actions(seed=9, t=2), envs[1].policy_actions(seed=9, t=2))
        for e, l in zip(envs, learners):
            l.step_pathwise(e.handle.onpolicy_batch(5, 0, 0, 64), draw=7)
        assert _same(learners[0].download("policy", ("grads",))["grads"], learners[1].download("policy", ("grads",))["grads"])
    finally:
        if fed is not None:
            fed.close()
        other["env"].close()
        _install(c)


# ---- refusals (check 10) -------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_valid_calls_their_bits(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    _install(c)
    learner, ql = _learners(env, lr=0.0)
    batch = h.onpolicy_batch(5, 0, 0, 64)
    learner.step_pathwise(batch, draw=1)
    want = _record(learner)
    kept = learner.download("policy")
    cfg = lambda **kw: _lib.pathwise_config(**dict(dict(alpha=0.2, bc_coef=0.5, stochastic=True, seed=ACTOR["pathwise_seed"], draw=1), **kw))
    step = lambda b=batch, n=64, **kw: h.learner_step_pathwise(b, n, cfg(**kw))
    _refused(lambda: step(struct_size=32), I, "struct_size 32")
    for k in ("alpha", "bc_coef"):
        for x in (math.nan, -0.5, math.inf):
            _refused(lambda: step(**{k: x}), I, "alpha and bc_coef must be finite and >= 0")
    bad = cfg()
    bad.stochastic = 2
    _refused(lambda: h.learner_step_pathwise(batch, 64, bad), I, "stochastic = 2")
    for n in (0, -3, (1 << 24) + 1):
        _refused(lambda: step(n=n), I, "outside 1 .. 2^24")
    _refused(lambda: step({k: x for k, x in batch.items() if k != "observations"}), I, "the batch lacks observations")
    _refused(lambda: step({k: x for k, x in batch.items() if k != "indices"}), I, "the batch lacks indices")
    step({k: x for k, x in batch.items() if k != "indices"}, bc_coef=0.0)      # (bc_coef = 0 reads no stored action)
    assert h._lib.gs_learner_step_pathwise(h._h, None, 64, ctypes.byref(cfg()), None) == I
    assert h._lib.gs_learner_pathwise_view(h._h, None, None) == I
    # the same bits after all of that
    learner.step_pathwise(batch, draw=1)
    _equal_records(want, _record(learner))
    # what needs preparation and learners refuses before any launch
    env.set_q(1, c["qs"][1])                                   # (installing twin 1 again ends its learner)
    _refused(lambda: step(), S, "no learner for Q network 1")
    env.set_q(0, None)
    env.set_q(1, None)
    _refused(lambda: step(), S, "no Q network is installed")
    env.set_policy(c["pol"], stochastic=True)                  # (and the policy's)
    for w in range(2):
        env.set_q(w, c["qs"][w])
    P.DeviceLearner(env, nets=("q1", "q2"), **HYPER)
    _refused(lambda: step(), S, "no learner for the policy")
    _refused(lambda: h.learner_pathwise_view(), S, "holds no pathwise step's arrays")
    # another normalisation on a twin
    mean, std = c["qs"][0].obs_mean, c["qs"][0].obs_std
    env.set_q(0, P.MLPQ(c["qs"][0].weights, c["qs"][0].biases, env.obs_dim, activation=c["activation"], obs_mean=mean, obs_std=std * 2.0))
    learner, ql = _learners(env, lr=0.0)
    _refused(lambda: step(), S, "differ from the normalisation of Q network 0")
    _install(c)
    learner, ql = _learners(env, lr=0.0)
    # minibatches prepared in float64, and a further rollout without preparation
    OnPolicyBatches(env, 185, policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS, dtype=np.float64).prepare()
    _refused(lambda: step(), S, "GS_COMPUTE_F32")
    env.reset(seed=3)
    rollout_device(env, c["T"], seed=7, reset=False)
    _refused(lambda: step(), S, "gs_onpolicy_prepare has not run on the last rollout")
    assert _same(learner.download("policy", ("params",))["params"], kept["params"]) and learner.info("policy")["step"] == 0
    # the same rollout and the same step again
    c["batches"] = _prepare(c, env)
    learner.step_pathwise(h.onpolicy_batch(5, 0, 0, 64), draw=1)
    _equal_records(want, _record(learner))
