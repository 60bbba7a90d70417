"""GPU: the conservative critic step (include/gridstep.h "the conservative critic step") -- a twin's regression
plus CQL's logsumexp penalty over the batch -- against the NumPy restatements of grid_fed_rl_gym_amd (``cql_grad_np``,
``cql_uniform_np``, ``cql_noise_np``, ``adam_np``, ``fedavg_np``).

Feeders, network recipe and hidden shapes are tests/test_gpu_pathwise.py's: 13-bus, T = 37 steps of B = 5 instances (185 rows), Q input
71 + 3; an 11-bus synthetic feeder; 123-bus, T = 3, B = 70, hidden 256, 256; and the 13-bus feeder with B = 10 (370 rows) for n = 342.
The minibatch sizes lay the three blocks of 3 n rows across the 32-row tiles (1, 33, 64, 65, 185), on either side of the 256-row
gradient segment (85, 86: 255 and 258 rows) and past the 1024 threads of the reductions (342: 1026 rows).

Bounds, none of them computed from the device:
  noise         within 1e-9 of ``cql_noise_np`` (section 12's bound for stochastic actions)
  S, lse        within 1e-13 relative of NumPy's on the device's q: 3 n positive terms each within 4 ulp, a tree of depth 10 and at most
                ceil(3 n / 1024) chained adds
  q, dW, db     within 4 E_ref of ``exact=True``, E_ref = the float32 restatement's own error on the same rows (section 15's rule with
                section 19's amendments, as tests/test_gpu_q_critics.py: below 32 rows E_ref from 32 rows, and the one-entry last bias
                gradient's E_ref at least 2^-24 sum_j |g_j| of the exact head gradient); both restatements are fed the device's candidate
                actions
  the rest      bit-equal: the uniform actions; m; the policy's actions and log-probabilities to ``_pathwise_sample`` fed the device's
                noise and pre-head values; targets; weights and loss terms to ``cql_grad_np`` fed the device's q, targets, m and S;
                qbar, penalty and loss; Adam; the installed image; rows under another n; twins; refusals; non-interference; FedAvg.
For n >= 33 the softmax check is kept from being vacuous by a condition on the RESTATEMENT's values: max_j p_j <= 0.25."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.federated import fedavg_np
from grid_fed_rl_gym_amd.learner import (_block_sum_np, _forward, _pathwise_sample, adam_np, cql_grad_np, cql_noise_np, cql_uniform_np,
                                         pathwise_tanh_np)
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
    "ieee13-large": ("ieee13", 10, 37, 14, [64, 64], "relu"),
}
GAMMA = 0.97
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, clip=0.2, ent_coef=0.01, max_grad_norm=0.5)
SEED = 0x5EED0123456789
ALPHA = 0.2
CW = 5.0
FIELDS = ["observations", "actions", "advantages", "returns", "values", "indices"]
NETS = ("q1", "q2")
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


def _install(c, qs=None, twins=(0, 1), pol=None, source="value"):
    """the networks as first installed (ends every learner of the handle), then the evaluations the Q learners' targets come from"""
    env = c["env"]
    env.set_policy(pol or c["pol"], stochastic=True)
    env.set_value(c["val"])
    for w in range(2):
        env.set_q(w, (qs or c["qs"])[w] if w in twins else None)
    env.handle.q_set_target_source(source)
    if "data" in c:
        _evaluate(c, source)


def _evaluate(c, source="value"):
    env = c["env"]
    if source == "value":
        P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
        P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
        c["td"] = env.handle.rollout_q_download(("td_target",))["td_target"].reshape(-1)
    else:
        P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=ALPHA, seed=17, draw=2)
        c["td"] = env.handle.rollout_q_next_download(("td_target",))["td_target"].reshape(-1)


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
    _evaluate(c)
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


def _twin(c, qs=None, twins=(0, 1), pol=None, source="value"):
    """another handle with the same networks installed, on which the rollout of ``c`` is repeated (its stored actions uploaded), the
    minibatches prepared and the targets evaluated; returns a case dict"""
    env = _env(c["feeder"], c["B"], c["ep"])
    t = {k: v for k, v in c.items() if k not in ("data", "td")}
    t["env"] = env
    _install(t, qs, twins, pol, source)
    env.reset(seed=3)
    rollout_device(env, c["T"], reset=False, actions=c["data"]["actions"])
    t["data"] = _rollout_arrays(env)
    assert _same(t["data"]["observations"], c["data"]["observations"]), "the repeated rollout collects the same observations"
    t["batches"] = _prepare(t, env)
    _evaluate(t, source)
    return t


def _learners(env, lr=None, twins=NETS, cw=CW, source="value", **kw):
    """(the policy's learner, which no test steps unless it says so, and the conservative twins' learner)"""
    hyper = HYPER if lr is None else dict(HYPER, lr=lr)
    pl = P.DeviceLearner(env, nets=("policy",), **hyper)
    ql = P.DeviceLearner(env, nets=twins, **hyper, q_target=source, conservative_weight=cw, conservative_seed=SEED, **kw)
    return pl, ql


def _host(batch):
    return {k: v.to_host() for k, v in batch.items() if v is not None and not isinstance(v, list)}


def _views(learner):
    v = learner.conservative_views()
    n, A = v["n"], v["action_dim"]
    out = {k: x.to_host() for k, x in v.items() if hasattr(x, "to_host")}
    flat, stride = out.pop("pre_head"), v["pre_head_stride"]
    out["pre_head"] = np.stack([flat[i * stride:i * stride + 2 * A] for i in range(n)])
    out["net"] = v["net"]
    return out


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


def _within(tag, what, got, exact, f32, rel_ref=None, floor=None):
    """section 19's bound with its two amendments (tests/test_gpu_q_critics.py ``_within``): below 32 rows E_ref comes from 32 rows,
    and E_ref of a one-entry tensor (the last bias gradient) is at least 2^-24 sum_j |g_j|, what rounding its terms to float32 costs"""
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


def _stored(c, idx):
    return c["data"]["actions"].reshape(c["B"] * c["T"], -1)[idx]


def _targets(c, idx):
    return c["td"][idx].astype(np.float32)


def _restate(c, layers, hb, v, exact, cw=CW, rows=slice(None), **kw):
    """``cql_grad_np`` on the minibatch ``hb`` with the candidate actions and targets of ``v`` (the device's, or a host stand-in's)"""
    return cql_grad_np(layers, hb["observations"][rows], _stored(c, hb["indices"])[rows], v["random_actions"][rows], v["policy_actions"][rows],
                       v["targets"][rows], cw, exact=exact, activation=c["activation"], **kw)


def _host_candidates(c, policy_layers, hb, draw, n):
    """the candidate actions and targets of a step the device did not take (an error scale below 32 rows): the host's own"""
    out = _forward(policy_layers, hb["observations"], c["activation"], False)[1][-1].astype(np.float64)
    a = _pathwise_sample(out, cql_noise_np(SEED, draw, n, out.shape[1] // 2))[3]
    return dict(random_actions=cql_uniform_np(SEED, draw, n, a.shape[1]), policy_actions=a, targets=_targets(c, hb["indices"]))


def _record(ql, net):
    rec = _views(ql)
    rec.update(grads=ql.download(net, ("grads",))["grads"], stats=ql.stats(net))
    return rec


def _equal_records(a, b, skip=("step",)):
    for k in a:
        if k == "stats":
            for s in a[k]:
                x, y = a[k][s], b[k][s]
                assert s in skip or x == y or (math.isnan(x) and math.isnan(y)), (s, x, y)
        elif k == "net":
            assert a[k] == b[k]
        else:
            assert _same(a[k], b[k]), k


# ---- the step against the restatements ---------------------------------------------------------------------------------------------------

# (name, n, conservative_weight, target source)
STEPS = ([("ieee13-relu", n, CW, "value") for n in (1, 33, 64, 65, 85, 86, 185)] +
         [("ieee13-relu", 65, 0.0, "value"), ("ieee13-relu", 33, CW, "policy"), ("ieee13-tanh40", 185, CW, "value"), ("ieee13-elu", 65, CW, "policy"),
          ("ieee123-relu", 65, CW, "value"), ("ieee13-single", 33, CW, "value"), ("scal11-relu", 65, CW, "value"), ("ieee13-large", 342, CW, "value")])


@pytest.mark.parametrize("name,n,cw,source", STEPS, ids=[f"{a}-n{b}-cw{int(w)}-{s}" for a, b, w, s in STEPS])
def test_three_conservative_steps_of_both_twins_against_the_restatements(prepared, name, n, cw, source):
    """Per step and twin: the candidate actions, the targets, the logsumexp's scalars, the softmax weights and loss terms, q and the
    twin's gradient at fresh parameters and after two steps, the statistics, Adam bit for bit over the three steps; then the online
    images against a twin handle on which ``learner.q(w)`` was installed.

    Observed on the MI355X: see DESIGN.md section 26 "Observed accuracy"."""
    c = prepared(name)
    env = c["env"]
    h = env.handle
    N = c["B"] * c["T"]
    try:
        _install(c, source=source)
        MISSED.clear()
        pl, ql = _learners(env, cw=cw, source=source)
        D, A = env.obs_dim, env.action_dim
        policy_layers = list(zip(*pl.parameters("policy")))
        policy_state = pl.download("policy")
        P_count = ql.info("q1")["param_count"]
        targets = [h.q_target_download(w, P_count) for w in range(2)]
        state = {net: ql.download(net) for net in NETS}
        for s in range(3):
            hb32 = _host(h.onpolicy_batch(5, s, 0, 32)) if n < 32 else None      # (first: a batch's arrays are the handle's until its next batch)
            batch = h.onpolicy_batch(5, s, 0, n)
            hb = _host(batch)
            seen = []
            for w, net in enumerate(NETS):
                layers = list(zip(*ql.parameters(net)))
                other = ql.download(NETS[1 - w])
                ql.step_conservative(batch, net, conservative_weight=cw, seed=SEED)      # (draw: the twin's steps taken, s for both)
                v = _views(ql)
                seen.append(v)
                tag = f"{name} n={n} step {s + 1} {net}"
                assert v["net"] == _lib.GS_LEARNER_Q + w and v["q"].shape == (3 * n,)
                # 1. the candidate actions and the targets
                assert _same(v["random_actions"], cql_uniform_np(SEED, s, n, A)), tag
                want_noise = cql_noise_np(SEED, s, n, A)
                e_noise = _err(v["policy_noise"], want_noise)
                print(f"{tag} noise: max |device - cql_noise_np| {e_noise:.3e}")
                assert e_noise <= 1e-9 and (n * A < 16 or np.std(v["policy_noise"]) > 0.1)
                a, lp = _pathwise_sample(v["pre_head"].astype(np.float64), v["policy_noise"])[3:]
                assert _differing(f"{tag} policy_actions", v["policy_actions"], a) and _differing(f"{tag} policy_log_probs", v["policy_log_probs"], lp)
                assert _same(v["targets"], _targets(c, hb["indices"])), tag
                # 2. the logsumexp: m bit-equal, S and lse within 1e-13 of NumPy's on the device's q, qbar in the device's order
                m, S_, lse, qbar = v["scalars"]
                q = v["q"]
                assert m == q.max() and not np.isnan(v["scalars"]).any()
                S_np = math.fsum(np.exp(q - m))
                lse_np = m + math.log(S_np)
                print(f"{tag} S: device {S_:.17g} NumPy {S_np:.17g} rel {abs(S_ - S_np) / S_np:.2e}; lse: device {lse:.17g} rel {abs(lse - lse_np) / abs(lse_np):.2e}")
                assert math.isclose(S_, S_np, rel_tol=1e-13) and math.isclose(lse, lse_np, rel_tol=1e-13)
                assert qbar == _block_sum_np(q[:n]) / n
                # 3. the head, fed the device's q, targets, m and S
                head = _restate(c, layers, hb, v, False, cw, q=q, scalars=v["scalars"])
                assert _differing(f"{tag} weights", v["weights"], head["weights"]) and _differing(f"{tag} loss_terms", v["loss_terms"], head["loss_terms"])
                # 4. q and the twin's gradient
                if s in (0, 2):
                    rel = {}
                    if n < 32:
                        assert hb32["indices"][0] == hb["indices"][0]
                        v32 = _host_candidates(c, policy_layers, hb32, s, 32)
                        ex32, lo32 = _restate(c, layers, hb32, v32, True, cw), _restate(c, layers, hb32, v32, False, cw)
                        rel["q"] = _err(lo32["q"], ex32["q"]) / float(np.max(np.abs(ex32["q"])))
                        for j in range(32):
                            r = slice(j, j + 1)
                            e1, f1 = _restate(c, layers, hb32, v32, True, cw, rows=r), _restate(c, layers, hb32, v32, False, cw, rows=r)
                            for l, ((ew, eb), (fw, fb)) in enumerate(zip(e1["grads"], f1["grads"])):
                                for what, e, f in ((f"dW[{l}]", ew, fw), (f"db[{l}]", eb, fb)):
                                    top = float(np.max(np.abs(e)))
                                    if top > 0.0:
                                        rel[what] = max(rel.get(what, 0.0), _err(f, e) / top)
                    exact, f32 = _restate(c, layers, hb, v, True, cw), _restate(c, layers, hb, v, False, cw)
                    if n >= 33:                               # a condition on the inputs: the softmax is spread over the batch
                        assert exact["weights"].max() <= 0.25, float(exact["weights"].max())
                    _within(tag, "q", q, exact["q"], f32["q"], rel.get("q"))
                    gW, gb = ql.gradients(net)
                    for l in range(len(layers)):
                        _within(tag, f"dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
                        floor = 2.0 ** -24 * math.fsum(np.abs(exact["backprop"]["deltas"][-1][:, 0])) if l == len(layers) - 1 else None
                        _within(tag, f"db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"), floor)
                    assert (n < 33 or np.std(exact["q"]) > 1e-3) and any(np.abs(g).max() > 0.0 for g in gW)
                # 5. the statistics: what the view holds, reduced
                st = ql.stats(net)
                assert st["step"] == s + 1 and math.isnan(st["approx_kl"]) and math.isnan(st["clip_fraction"]) and math.isnan(st["entropy"])
                assert math.isclose(st["value_loss"], math.fsum(v["loss_terms"]) / n, rel_tol=1e-12, abs_tol=1e-300)
                assert st["surrogate"] == lse - qbar and st["loss"] == st["value_loss"] + cw * st["surrogate"]
                # 6. Adam, on this twin alone
                g = ql.download(net, ("grads",))["grads"]
                p, mm, vv = adam_np(state[net]["params"], g, state[net]["m"], state[net]["v"], s + 1, HYPER, st["grad_norm"])
                got = ql.download(net)
                assert np.array_equal(got["params"], p) and np.array_equal(got["m"], mm) and np.array_equal(got["v"], vv), tag
                now = ql.download(NETS[1 - w])
                assert all(_same(now[k], other[k]) for k in now), "the other twin is not written"
            state = {net: ql.download(net) for net in NETS}
            # Q1 then Q2 with the same seed and draw see the same candidates
            assert _same(seen[0]["random_actions"], seen[1]["random_actions"]) and _same(seen[0]["policy_actions"], seen[1]["policy_actions"])
            assert _same(seen[0]["targets"], seen[1]["targets"]) and not _same(seen[0]["q"], seen[1]["q"])
        assert not MISSED, MISSED
        # the policy and the target images were read, not written
        now = pl.download("policy")
        assert all(_same(now[k], policy_state[k]) for k in now) and pl.info("policy")["step"] == 0
        assert all(_same(h.q_target_download(w, P_count), targets[w]) for w in range(2))
        _refused(lambda: ql.views("q1"), S, "holds no step's arrays")
        # 7. the images Adam rewrote, against a fresh install of the same parameters on a twin handle
        if (name, n) in (("ieee13-relu", 65), ("ieee123-relu", 65), ("ieee13-single", 33)) and cw and source == "value":
            trained = [ql.q(w) for w in range(2)]
            assert not np.array_equal(trained[0].weights[0].astype(np.float32), c["qs"][0].weights[0].astype(np.float32))
            _evaluate(c)
            mine = h.rollout_q_download(("q",))["q"]["online"]
            t = _twin(c, qs=trained)
            try:
                theirs = t["env"].handle.rollout_q_download(("q",))["q"]["online"]
                assert all(_same(mine[w], theirs[w]) for w in range(2))
            finally:
                t["env"].close()
    finally:
        _install(c)


def test_a_rows_q_does_not_depend_on_the_batch_it_lies_in(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    _install(c)
    pl, ql = _learners(env, lr=0.0)
    out = []
    for n in (65, 185):
        ql.step_conservative(h.onpolicy_batch(5, 0, 0, n), "q1", draw=3)
        out.append(_views(ql))
    a, b = out
    for k in ("random_actions", "policy_actions", "policy_noise", "policy_log_probs", "targets"):
        assert _same(a[k], b[k][:65]), k
    for block in range(3):                                    # data | uniform | policy
        assert _same(a["q"][65 * block:65 * block + 65], b["q"][185 * block:185 * block + 65]), block
    assert not _same(a["weights"][:65], b["weights"][:65])    # (the softmax runs over the batch)


def test_determinism_twins_draws_seeds_and_the_deterministic_candidates(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    _install(c)
    pl, ql = _learners(env, lr=0.0)
    batch = h.onpolicy_batch(5, 0, 0, 185)
    ql.step_conservative(batch, "q1", draw=1)
    a = _record(ql, "q1")
    ql.step_conservative(batch, "q1", draw=1)
    _equal_records(a, _record(ql, "q1"))                      # the same call twice (lr = 0: the same parameters)
    ql.step_conservative(batch, "q2", draw=1)
    b = _record(ql, "q2")
    assert _same(a["random_actions"], b["random_actions"]) and _same(a["policy_actions"], b["policy_actions"]) and b["net"] == a["net"] + 1
    ql.step_conservative(batch, "q1", draw=2)
    other = _views(ql)
    for k in ("random_actions", "policy_noise", "policy_actions"):
        assert not np.array_equal(other[k], a[k]), k
    ql.step_conservative(batch, "q1", draw=1, seed=SEED + 1)
    other = _views(ql)
    assert not np.array_equal(other["random_actions"], a["random_actions"]) and not np.array_equal(other["policy_noise"], a["policy_noise"])
    ql.step_conservative(batch, "q1", draw=1, stochastic=False)
    det = _views(ql)
    assert not det["policy_noise"].any() and not np.signbit(det["policy_noise"]).any()
    assert _same(det["policy_actions"], pathwise_tanh_np(det["pre_head"][:, :env.action_dim].astype(np.float64)))
    assert _same(det["random_actions"], a["random_actions"])
    t = _twin(c)
    try:                                                      # two handles
        tl, tq = _learners(t["env"], lr=0.0)
        tq.step_conservative(t["env"].handle.onpolicy_batch(5, 0, 0, 185), "q1", draw=1)
        _equal_records(a, _record(tq, "q1"))
    finally:
        t["env"].close()
    # one twin alone, with the bits it has beside the other
    for w in range(2):
        _install(c, twins=(w,))
        l1, q1 = _learners(env, lr=0.0, twins=(NETS[w],))
        q1.step_conservative(h.onpolicy_batch(5, 0, 0, 185), NETS[w], draw=1)
        _equal_records(a if w == 0 else b, _record(q1, NETS[w]))
    _install(c)


def test_the_scaled_twin_takes_the_overflow_branch_without_a_nan(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    n = 185
    ws = [w.copy() for w in c["qs"][0].weights]
    ws[-1] = ws[-1] * 2000.0
    scaled = P.MLPQ(ws, c["qs"][0].biases, env.obs_dim, activation=c["activation"], obs_mean=c["qs"][0].obs_mean, obs_std=c["qs"][0].obs_std)
    try:
        _install(c, qs=[scaled, c["qs"][1]])
        pl, ql = _learners(env)
        layers = list(zip(*ql.parameters("q1")))
        batch = h.onpolicy_batch(5, 0, 0, n)
        hb = _host(batch)
        ql.step_conservative(batch, "q1")
        v = _views(ql)
        q = v["q"]
        host = _restate(c, layers, hb, v, False, q=q, scalars=v["scalars"])
        below = q - q.max() < -700.0
        print(f"q spans {q.min():.1f} .. {q.max():.1f}; {int(below.sum())} of {q.size} rows lie more than 700 below the maximum")
        assert q.max() - q.min() > 1400.0 and below.sum() > 0
        assert _same(v["weights"], host["weights"]) and np.all(v["weights"][below] == 0.0) and np.all(v["weights"][~below] > 0.0)
        assert np.array_equal(below, host["weights"] == 0.0)
        got = ql.download("q1")
        st = ql.stats("q1")
        assert all(np.isfinite(got[k]).all() for k in got) and got["grads"].any()
        assert all(math.isfinite(st[k]) for k in ("loss", "surrogate", "value_loss", "grad_norm")) and np.isfinite(v["scalars"]).all()
        assert math.isclose(v["scalars"][2], float(np.logaddexp.reduce(q)), rel_tol=1e-13)
    finally:
        _install(c)


# ---- non-interference ------------------------------------------------------------------------------------------------------------------

def _pathwise_record(al):
    v = al.pathwise_views()
    out = {k: x.to_host() for k, x in v.items() if hasattr(x, "to_host") and k != "pre_head"}      # (pre_head: the shared scratch)
    for k in ("q", "dq_da"):
        out[k + "0"], out[k + "1"] = (x.to_host() for x in v[k])
    return out


def test_a_conservative_step_leaves_the_rest_of_the_handle_alone(prepared):
    """The other twin, the policy, both target images and the pathwise step's arrays keep their bits; a plain Q step and a pathwise
    step after conservative steps are those of a handle that never called the new entry (lr = 0 keeps the parameters' bits, and a
    new ``DeviceLearner`` starts Adam afresh)."""
    c = prepared("ieee13-elu")
    outs = []
    for conservative_steps in (2, 0):
        t = _twin(c)
        env = t["env"]
        h = env.handle
        try:
            if conservative_steps:
                al = P.DeviceLearner(env, nets=("policy",), **dict(HYPER, lr=0.0), policy_loss="pathwise", alpha=ALPHA, pathwise_seed=3)
                ql = P.DeviceLearner(env, nets=NETS, **dict(HYPER, lr=0.0), conservative_weight=CW, conservative_seed=SEED)
                al.step_pathwise(h.onpolicy_batch(5, 0, 0, 64), draw=4)
                kept = _pathwise_record(al)
                P_count = ql.info("q1")["param_count"]
                before = dict(policy=al.download("policy"), q2=ql.download("q2"), targets=[h.q_target_download(w, P_count) for w in range(2)])
                for s in range(conservative_steps):
                    ql.step_conservative(h.onpolicy_batch(5, s, 0, 185 - s), "q1")
                now = _pathwise_record(al)
                assert all(_same(now[k], kept[k]) for k in kept)
                for net, learner in (("policy", al), ("q2", ql)):
                    got = learner.download(net)
                    assert all(_same(got[k], before[net][k]) for k in got) and learner.info(net)["step"] == (1 if net == "policy" else 0), net
                assert all(_same(h.q_target_download(w, P_count), before["targets"][w]) for w in range(2))
                assert ql.info("q1")["step"] == conservative_steps
            d = {}
            plain = P.DeviceLearner(env, nets=("policy",) + NETS, **HYPER, policy_loss="pathwise", alpha=ALPHA, pathwise_seed=3)
            for net in NETS:
                h.learner_step(net, h.onpolicy_batch(5, 0, 0, 65), 65)
                d[f"{net}.loss_terms"] = plain.views(net)["loss_terms"].to_host()
            plain.step_pathwise(h.onpolicy_batch(5, 0, 0, 65), draw=1)
            d.update({f"pathwise.{k}": x for k, x in _pathwise_record(plain).items()})
            for net in plain.nets:
                d.update({f"{net}.{k}": x for k, x in plain.download(net).items()})
            outs.append(d)
        finally:
            env.close()
    for k in outs[0]:
        assert _same(outs[0][k], outs[1][k]), k
    assert outs[0]["policy.grads"].any() and outs[0]["q1.grads"].any()


def test_a_federated_round_over_two_conservatively_trained_twins_is_fedavg_np(prepared):
    c = prepared("ieee13-relu")
    _install(c)
    other = _twin(c)
    fed = None
    try:
        envs = (c["env"], other["env"])
        pairs = [_learners(e) for e in envs]
        learners = [p[1] for p in pairs]
        fed = P.FederatedLearners(learners)
        for k, (e, l) in enumerate(zip(envs, learners)):
            for s in range(1 + k):                                      # (different numbers of local steps: different parameters)
                l.step(e.handle.onpolicy_batch(5, s, 0, 64 + k))
        g0 = {net: fed.global_parameters(net) for net in NETS}
        kept = {net: [l.download(net) for l in learners] for net in NETS}
        out = fed.round(weights=[40.0, 25.0], clip_norm=0.02)
        for net in NETS:
            assert not np.array_equal(kept[net][0]["params"], kept[net][1]["params"])
            agg = fedavg_np(g0[net], [k["params"] for k in kept[net]], [40.0, 25.0], norms=out[net]["norms"], clip_norm=0.02)
            for l in learners:
                assert _same(l.download(net, ("params",))["params"], agg), net
        # the aggregate reached the installed images: a further conservative step is the same on both clients
        for e, l in zip(envs, learners):
            l.step_conservative(e.handle.onpolicy_batch(5, 0, 0, 64), "q1", draw=7)
        assert _same(learners[0].download("q1", ("grads",))["grads"], learners[1].download("q1", ("grads",))["grads"])
        assert learners[0].download("q1", ("grads",))["grads"].any()
    finally:
        if fed is not None:
            fed.close()
        other["env"].close()
        _install(c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_valid_calls_their_bits(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    h = env.handle
    Q1 = _lib.GS_LEARNER_Q
    try:
        _install(c)
        pl, ql = _learners(env, lr=0.0)
        batch = h.onpolicy_batch(5, 0, 0, 64)
        ql.step_conservative(batch, "q1", draw=1)
        want = _record(ql, "q1")
        kept = ql.download("q1")
        cfg = lambda **kw: _lib.conservative_config(**dict(dict(conservative_weight=CW, stochastic=True, seed=SEED, draw=1), **kw))
        step = lambda b=batch, n=64, net=Q1, **kw: h.learner_step_conservative(net, b, n, cfg(**kw))
        _refused(lambda: step(struct_size=40), I, "struct_size 40")
        for net in (_lib.GS_LEARNER_POLICY, _lib.GS_LEARNER_VALUE, Q1 + 2, -1):
            with pytest.raises((PowerFlowError, ValueError)) as e:
                h._check(h._lib.gs_learner_step_conservative(h._h, net, ctypes.byref(_lib.gs_onpolicy_batch_out()), 64, ctypes.byref(cfg()), None))
            assert f"libgridstep error {I}:" in str(e.value) and "is not GS_LEARNER_Q + {0, 1}" in str(e.value)
        for x in (math.nan, -0.5, math.inf):
            _refused(lambda: step(conservative_weight=x), I, "conservative_weight must be finite and >= 0")
        bad = cfg()
        bad.stochastic = 2
        _refused(lambda: h.learner_step_conservative(Q1, batch, 64, bad), I, "stochastic = 2")
        for n in (0, -3, (1 << 24) // 3 + 1):
            _refused(lambda: step(n=n), I, "outside 1 .. 2^24 / 3")
        _refused(lambda: step({k: x for k, x in batch.items() if k != "observations"}), I, "the batch lacks observations")
        _refused(lambda: step({k: x for k, x in batch.items() if k != "indices"}), I, "the batch lacks indices")
        assert h._lib.gs_learner_step_conservative(h._h, Q1, None, 64, ctypes.byref(cfg()), None) == I
        assert h._lib.gs_learner_conservative_view(h._h, None, None) == I
        # the same bits after all of that
        ql.step_conservative(batch, "q1", draw=1)
        _equal_records(want, _record(ql, "q1"))
        # what needs learners, a loss, targets and preparation refuses before any launch
        ql.set_loss("q1", "expectile", expectile=0.7)
        _refused(lambda: step(), S, "must be GS_LOSS_DEFAULT")
        ql.set_loss("q1", "mse")
        h.q_set_target_source("policy")
        _refused(lambda: step(), S, "gs_rollout_evaluate_q_next has not run")
        h.q_set_target_source("value")
        env.set_q(0, c["qs"][0])                                  # (installing twin 0 again ends its learner, and the evaluation)
        _refused(lambda: step(), S, "no learner for Q network 0")
        _refused(lambda: h.learner_conservative_view(), S, "holds a conservative step's arrays")
        P.DeviceLearner(env, nets=("q1",), **HYPER)
        _refused(lambda: step(), S, "gs_rollout_evaluate_q has not run")
        _evaluate(c)
        env.set_policy(c["pol"], stochastic=True)                 # (and the policy's)
        _refused(lambda: step(), S, "no learner for the policy")
        _evaluate(c)
        # another normalisation on the twin
        mean, std = c["qs"][0].obs_mean, c["qs"][0].obs_std
        env.set_q(0, P.MLPQ(c["qs"][0].weights, c["qs"][0].biases, env.obs_dim, activation=c["activation"], obs_mean=mean, obs_std=std * 2.0))
        pl, ql = _learners(env, lr=0.0)
        _evaluate(c)
        _refused(lambda: step(), S, "differ from the normalisation of Q network 0")
        _install(c)
        pl, ql = _learners(env, lr=0.0)
        # minibatches prepared in float64, and a further rollout without preparation
        OnPolicyBatches(env, 185, policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS, dtype=np.float64).prepare()
        _refused(lambda: step(), S, "GS_COMPUTE_F32")
        env.reset(seed=3)
        rollout_device(env, c["T"], seed=7, reset=False)
        _refused(lambda: step(), S, "gs_onpolicy_prepare has not run on the last rollout")
        assert _same(ql.download("q1", ("params",))["params"], kept["params"]) and ql.info("q1")["step"] == 0
        # the same rollout and the same step again
        c["batches"] = _prepare(c, env)
        _evaluate(c)
        ql.step_conservative(h.onpolicy_batch(5, 0, 0, 64), "q1", draw=1)
        _equal_records(want, _record(ql, "q1"))
    finally:
        env.reset(seed=3)
        rollout_device(env, c["T"], seed=7, reset=False)
        c["batches"] = _prepare(c, env)
        _install(c)
