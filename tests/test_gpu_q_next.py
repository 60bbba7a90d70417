"""GPU: policy-action TD targets (include/gridstep.h "policy-action TD targets") -- the installed policy over the
next states of a rollout (``gs_k_policy_rows_f32``), the target twins on its actions, the Bellman target and the Q learner that
regresses on it, against the NumPy restatements of grid_fed_rl_gym_amd (``policy_rows_np``, ``q_next_noise_np``, ``q_rollout_np``,
``td_policy_np``, ``value_grad_np``, ``adam_np``).

The datasets and shapes are section 22's (tests/test_gpu_q_critics.py): a RANDOM-ACTION rollout.  13-bus: T = 37, B = 5 (N = 185 rows:
tiles of 64, 64 and 57), obs_dim 71 odd, action_dim 3 (2 A = 6: the last layer's one column tile is not full), ``episode_length`` 14
under voltage limits (0.98, 1.02): episodes end at the time limit (bit 0) and after violations (bit 1), both asserted.  123-bus: T = 3,
B = 70, hidden 256, 256; 684 observation columns are 43 blocks in three panels, and A = 8 makes the head's column tile exactly full (2 A = 16).  An
11-bus synthetic feeder (obs_dim 113, action_dim 4): T = 9, B = 9.  A 40-bus synthetic feeder (obs_dim 979 odd, 62 blocks in three
panels; action_dim 11: 2 A = 22 is TWO head tiles, the second not full): T = 18, B = 9, ``episode_length`` 2 -- 162 rows and 81
terminal rows, because E_ref is NumPy's own float32 error and measures a float32 chain only where NumPy's product takes its blocked
path: at 979 columns a plain ascending float32 chain (restated on the host, no device involved; 20 draws of N(0, 1) rows) lies at 5.5
E_ref in the median and up to 8.2 with 6 or 12 rows, at 2.1 and up to 3.0 with 81.  The policy and the twins of a case share its hidden widths and activation.

Bounds, none of them computed from the device:
  next_pre_head, q_next   within 4 E_ref, E_ref = the float32 restatement's own error against ``exact=True`` on the same rows (the
                          project's bound since section 19)
  the noise               within 1e-9 of ``q_next_noise_np`` (the host's log, sin and cos are a library's)
  everything else         bit-equal: actions and log-probabilities to ``policy_rows_np`` fed the device's pre-head values and the
                          device's noise; q_next_min, td_target and the terminal arrays to ``td_policy_np`` fed the device's arrays;
                          rows under another B and on a second handle; Adam; the learner under GS_Q_TARGET_VALUE afterwards."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.learner import adam_np, pathwise_tanh_np, value_grad_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, policy_rows_np, q_next_noise_np, q_rollout_np, rollout_device, td_policy_np

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like, "scal11": lambda: P.scalable_like(11, seed=1),
           "scal40": lambda: P.scalable_like(40, seed=1)}
SOLVER = {"scal11": "nr", "scal40": "nr"}       # (feeders with loops)
# name: (feeder, B, T, episode_length, hidden widths, activation)
CASES = {
    "ieee13-relu": ("ieee13", 5, 37, 14, [64, 64], "relu"),
    "ieee13-tanh40": ("ieee13", 5, 37, 14, [40, 40], "tanh"),
    "ieee13-elu": ("ieee13", 5, 37, 14, [64, 64], "elu"),
    "ieee123-relu": ("ieee123", 70, 3, 2, [256, 256], "relu"),
    "ieee13-single": ("ieee13", 5, 37, 14, [], "relu"),
    "scal11-relu": ("scal11", 9, 9, 3, [64, 64], "relu"),
    "scal40-relu": ("scal40", 9, 18, 2, [64, 64], "relu"),
}
GAMMA, ALPHA, SEED, DRAW = 0.97, 0.2, 0x5EED0123456789, 4
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


def _layers(dims, seed, last_scale=1.0):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    ws[-1] *= last_scale
    return ws, bs


def _networks(feeder, D, A, hidden, activation):
    mean, std = _normalisation(feeder)
    # (the last layer scaled down: mean and log_std stay moderate, so the actions keep away from saturation)
    pol = P.MLPPolicy(*_layers([D] + hidden + [2 * A], 1, 0.3), activation=activation, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    val = P.MLPValue(*_layers([D, 64, 1], 2), activation="relu", obs_mean=mean, obs_std=std)
    qs = [P.MLPQ(*_layers([D + A] + hidden + [1], 20 + w), D, activation=activation, obs_mean=mean, obs_std=std) for w in range(2)]
    return pol, val, qs


def _install(c, qs=None, twins=(0, 1), pol=None):
    """the networks as first installed: ends every learner of the handle"""
    env = c["env"]
    env.set_policy(pol or c["pol"], stochastic=True)
    env.set_value(c["val"])
    for w in twins:
        env.set_q(w, (qs or c["qs"])[w])


def _rollout_arrays(env):
    h = env.handle
    d = h.rollout_download(want=("observations", "actions", "rewards", "terminals"))
    dev = h.rollout_device_arrays()
    d["terminal_index"] = dev["terminal_index"].to_host()
    d["terminal_obs"] = dev["terminal_obs"].to_host()
    d["next_observations"] = dev["obs_seq"].to_host()[1:]
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
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)      # (what gs_onpolicy_prepare needs; the new entry does not)
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


def _twin(c, B=None, twins=(0, 1), pol=None, qs=None):
    """another handle with the networks of ``c`` (or ``pol`` / ``qs``) installed, on which the rollout of ``c`` is repeated (the first
    ``B`` instances, their stored actions uploaded); returns (env, its rollout's arrays)"""
    B = B or c["B"]
    env = _env(c["feeder"], B, c["ep"])
    _install(dict(c, env=env), qs, twins, pol)
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


def _close(tag, what, got, exact, f32):
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    WORST[what] = max(WORST.get(what, 0.0), ratio if math.isfinite(ratio) else 1e9)
    assert e_ref > 0.0 and e_dev <= 4.0 * e_ref, (tag, what, e_dev, e_ref)


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
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def _evaluate(env, mask=3, alpha=ALPHA, stochastic=True, seed=SEED, draw=DRAW, **kw):
    P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=alpha, bootstrap=mask, stochastic=stochastic, seed=seed, draw=draw, **kw)
    return env.handle.rollout_q_next_download()


def _td(d, got, mask, alpha, shift=0.0, scale=1.0):
    """td_policy_np fed the device's own arrays"""
    return td_policy_np(d["rewards"], got["next_log_probs"], got["q_next_min"], d["terminals"], got["term_q_min"], d["terminal_index"], GAMMA, alpha, mask,
                        shift, scale, terminal_log_probs=got["term_log_probs"])


def _assert_equal_evaluations(a, da, b, db, B):
    """two downloads bit for bit; the terminal arrays entry by entry through (t, b): the list is appended in no particular order"""
    order = lambda d: np.argsort(d["terminal_index"][:, 0].astype(np.int64) * B + d["terminal_index"][:, 1], kind="stable")
    oa, ob = order(da), order(db)
    assert np.array_equal(da["terminal_index"][oa], db["terminal_index"][ob])
    for k, v in a.items():
        for x, y in zip(v, b[k]) if isinstance(v, list) else [(v, b[k])]:
            if k.startswith("term_"):
                x, y = x[oa], y[ob]
            assert _same(x, y), k


def _min(qs):
    qs = [q for q in qs if not np.isnan(q).all()]
    return qs[0].copy() if len(qs) == 1 else np.fmin(qs[0], qs[1])


# ---- evaluation --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_policy_rows_target_twins_and_targets_against_the_restatements(prepared, name):
    """Observed on the MI355X: see DESIGN.md section 25 "Observed accuracy"."""
    c = prepared(name)
    env, d, T, B, pol = c["env"], c["data"], c["T"], c["B"], c["pol"]
    D, A = env.obs_dim, env.action_dim
    flags = d["terminals"]
    if c["feeder"] == "ieee13":
        assert (D, A) == (71, 3)
        assert (flags == 1).any() and ((flags & 2) != 0).any(), "the dataset ends episodes under both done bits"
    elif c["feeder"] == "ieee123":
        assert D == 684 and A == 8 and (flags != 0).any()      # 2 A = 16: the head's column tile is exactly full
    elif c["feeder"] == "scal40":
        assert D == 979 and A == 11 and (flags != 0).sum() >= 81     # 2 A = 22: two head tiles
    else:
        assert (flags != 0).any()
    _install(c)
    P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=ALPHA, bootstrap=3, stochastic=True, seed=SEED, draw=DRAW)
    view = env.handle.rollout_q_next_arrays()
    got = env.handle.rollout_q_next_download()
    n = len(d["terminal_index"])
    assert view["installed"] == (0, 1) and view["rows_per_tile"] == 64 and view["n_terminal"] == n and n > 0
    assert view["next_pre_head"].shape == (T, B, 2 * A) and view["next_actions"].shape == (T, B, A) and view["term_value"].shape == (n,)
    for k in ("next_pre_head", "next_actions", "next_noise", "next_log_probs", "q_next_min", "td_target", "term_pre_head", "term_actions", "term_noise",
              "term_log_probs", "term_q_min", "term_value"):
        assert _same(view[k].to_host(), got[k]), k
    index = {"next": np.arange(T * B), "term": d["terminal_index"][:, 0].astype(np.int64) * B + d["terminal_index"][:, 1]}
    obs = {"next": d["next_observations"].reshape(T * B, D), "term": d["terminal_obs"]}
    for part, rows in (("next", T * B), ("term", n)):
        key = lambda k: f"{part}_{k}"
        pre = got[key("pre_head")].reshape(rows, 2 * A)
        act, eps, lp = got[key("actions")].reshape(rows, A), got[key("noise")].reshape(rows, A), got[key("log_probs")].reshape(rows)
        exact, f32 = policy_rows_np(pol, obs[part], None, exact=True)[0], policy_rows_np(pol, obs[part], None)[0]
        _close(name, f"{part}_pre_head", pre, exact, f32)
        assert _err(eps, q_next_noise_np(SEED, DRAW, index[part], A, terminal=part == "term")) <= 1e-9
        _, want_a, want_lp = policy_rows_np(pol, obs[part], eps, pre_head=pre)
        assert _same(act, want_a) and _same(lp, want_lp), part
        assert np.std(act) > 1e-2 and (np.abs(act) < 1.0).all()
        for w in range(2):
            q = (got["q_next"][w] if part == "next" else got["term_q"][w]).reshape(rows)
            o3, a3 = obs[part][None], act[None]
            _close(name, f"{part}_q[{w}]", q, q_rollout_np(c["qs"][w], o3, a3, exact=True)[0], q_rollout_np(c["qs"][w], o3, a3)[0])
    assert not np.array_equal(got["q_next"][0], got["q_next"][1])
    assert _same(got["q_next_min"], np.fmin(got["q_next"][0], got["q_next"][1])) and _same(got["term_q_min"], np.fmin(got["term_q"][0], got["term_q"][1]))
    assert _same(got["term_value"], got["term_q_min"] - ALPHA * got["term_log_probs"])
    assert _same(got["td_target"], _td(d, got, 3, ALPHA))


@pytest.mark.parametrize("mask", [0, 1, 3])
@pytest.mark.parametrize("alpha", [0.0, 0.2])
def test_minimum_and_td_target_bit_for_bit(prepared, mask, alpha):
    for name in ("ieee13-relu", "ieee123-relu"):
        c = prepared(name)
        env, d = c["env"], c["data"]
        _install(c)
        got = _evaluate(env, mask, alpha)
        if mask == 0:
            assert np.isnan(got["term_value"]).all() and env.handle.rollout_q_next_arrays()["term_value"] is None
            assert _same(got["td_target"], td_policy_np(d["rewards"], got["next_log_probs"], got["q_next_min"], d["terminals"], [], np.zeros((0, 2)), GAMMA, alpha, 0))
            ended = (d["terminals"] != 0).astype(np.float64)      # the reference's form
            assert _same(got["td_target"], d["rewards"] + GAMMA * ((1 - ended) * (got["q_next_min"] - alpha * got["next_log_probs"])))
        else:
            assert _same(got["term_value"], got["term_q_min"] - alpha * got["term_log_probs"])
            assert _same(got["td_target"], _td(d, got, mask, alpha)), (name, mask, alpha)
            hit = (d["terminals"] & mask) != 0
            assert hit.any() and (got["td_target"][hit] != d["rewards"][hit]).any()
        assert _same(got["q_next_min"], _min(got["q_next"]))
        shifted = _evaluate(env, mask, alpha, reward_shift=0.5, reward_scale=0.25)
        want = _td(d, shifted, mask, alpha, 0.5, 0.25) if mask else td_policy_np(d["rewards"], shifted["next_log_probs"], shifted["q_next_min"], d["terminals"], [],
                                                                                 np.zeros((0, 2)), GAMMA, alpha, 0, 0.5, 0.25)
        assert _same(shifted["td_target"], want) and _same(shifted["next_actions"], got["next_actions"])
    # one twin alone: the same bits, and the minimum is that twin
    c = prepared("ieee13-relu")
    env, d = c["env"], c["data"]
    both = _evaluate(env, mask, alpha)
    env.set_q(0, None)
    one = _evaluate(env, mask, alpha)
    assert np.isnan(one["q_next"][0]).all() and _same(one["q_next"][1], both["q_next"][1]) and _same(one["q_next_min"], both["q_next"][1])
    assert env.handle.rollout_q_next_arrays()["installed"] == (1,)
    if mask:
        assert _same(one["term_q_min"], both["term_q"][1]) and _same(one["td_target"], _td(d, one, mask, alpha))
    _install(c)


@pytest.mark.parametrize("name,B2", [("ieee13-relu", 7), ("ieee13-tanh40", 3), ("ieee123-relu", 37)])
def test_a_rows_outputs_do_not_depend_on_the_batch_it_lies_in(prepared, name, B2):
    """The same OBSERVATION rows under another B: with the deterministic head every output of a row is the same bits (the noise of a
    row is its transition's, t * B + b, which another B moves).  A second handle of the same B gives the sampled rows' bits too."""
    c = prepared(name)
    _install(c)
    want = _evaluate(c["env"], stochastic=False)
    env, d = _twin(c, B=B2)
    try:
        nb = min(B2, c["B"])
        assert _same(d["next_observations"][:, :nb], c["data"]["next_observations"][:, :nb]), "the repeated rollout collects the same observations"
        got = _evaluate(env, stochastic=False)
        for k in ("next_pre_head", "next_actions", "next_log_probs", "q_next_min"):
            assert _same(got[k][:, :nb], want[k][:, :nb]), k
        for w in range(2):
            assert _same(got["q_next"][w][:, :nb], want["q_next"][w][:, :nb]), w
    finally:
        env.close()
    if name == "ieee13-relu":
        want = _evaluate(c["env"])
        env, d = _twin(c)
        try:
            _assert_equal_evaluations(want, c["data"], _evaluate(env), d, c["B"])
        finally:
            env.close()


def test_draw_and_seed_move_the_sampled_rows_and_nothing_deterministic(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    _install(c)
    base = _evaluate(env)
    assert _same(_evaluate(env)["td_target"], base["td_target"]) and _same(_evaluate(env)["next_actions"], base["next_actions"])
    for kw in (dict(draw=DRAW + 1), dict(seed=SEED + 1)):
        other = _evaluate(env, **kw)
        for k in ("next_noise", "next_actions", "next_log_probs", "td_target", "term_noise", "term_actions"):
            assert not np.array_equal(other[k], base[k]), (kw, k)
        assert _same(other["next_pre_head"], base["next_pre_head"])
    det = _evaluate(env, stochastic=False)
    assert not det["next_noise"].any() and not np.signbit(det["next_noise"]).any() and not det["term_noise"].any()
    A = env.action_dim
    assert _same(det["next_actions"], pathwise_tanh_np(det["next_pre_head"][..., :A].astype(np.float64)))
    assert _same(det["term_actions"], pathwise_tanh_np(det["term_pre_head"][..., :A].astype(np.float64)))
    for kw in (dict(draw=DRAW + 1), dict(seed=SEED + 1)):
        other = _evaluate(env, stochastic=False, **kw)
        for k, v in det.items():
            for a, b in zip(v, other[k]) if isinstance(v, list) else [(v, other[k])]:
                assert _same(a, b), (kw, k)


# ---- the Q learner on the policy-action target ---------------------------------------------------------------------------------------

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


def _q_steps(env, steps, n, q_target):
    """(parameters, gradients) of both twins after every one of ``steps`` steps of a fresh Q learner"""
    learner = P.DeviceLearner(env, nets=("q1", "q2"), **HYPER, q_target=q_target)
    out = []
    for s in range(steps):
        learner.step(env.handle.onpolicy_batch(5, s, 0, n))
        out.append([learner.download(net, ("params", "grads", "m", "v")) for net in ("q1", "q2")])
    return learner, out


@pytest.mark.parametrize("n", [1, 33, 64, 65, 185])
def test_three_q_steps_on_the_policy_action_target(prepared, n):
    """Both twins regress on float32(td_target[idx]) of gs_rollout_evaluate_q_next over [obs | float32(act)], WITHOUT
    gs_rollout_evaluate_q: gradients at fresh parameters and after two steps within 4 E_ref, Adam bit for bit; then the same
    learner under GS_Q_TARGET_VALUE gives the bits of a handle that never called the new entries.

    Observed on the MI355X: see DESIGN.md section 25 "Observed accuracy"."""
    name = "ieee13-relu"
    c = prepared(name)
    env = c["env"]
    h = env.handle
    _install(c)
    td = _evaluate(env)["td_target"].reshape(-1)
    MISSED.clear()
    nets = ("q1", "q2")
    learner = P.DeviceLearner(env, nets=nets, **HYPER, q_target="policy")
    assert h.q_get_target_source() == "policy" and learner.q_target == "policy"
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
                dlt = exact["values"] - y.astype(np.float64)
                for l in range(len(layers)):
                    _within(tag, f"dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], rel.get(f"dW[{l}]"))
                    floor = 2.0 ** -24 * math.fsum(np.abs((2.0 * dlt) / n)) if l == len(layers) - 1 else None
                    _within(tag, f"db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], rel.get(f"db[{l}]"), floor)
            g = learner.download(net, ("grads",))["grads"]
            st = learner.stats(net)
            assert st["step"] == s + 1
            p, m, v = adam_np(state[net]["params"], g, state[net]["m"], state[net]["v"], s + 1, HYPER, st["grad_norm"])
            got = learner.download(net)
            assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v), (tag,)
            state[net] = got
    assert not MISSED, MISSED
    # back under GS_Q_TARGET_VALUE: the bits of a handle that never called the new entries
    if n in (33, 185):
        learner.set_q_target("value")
        assert h.q_get_target_source() == "value"
        _install(c)
        P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
        P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
        _, got = _q_steps(env, 2, n, "value")
        twin, d2 = _twin(c)
        try:
            P.evaluate_rollout(twin, gamma=GAMMA, lam=0.95, bootstrap=3)
            P.evaluate_rollout_q(twin, gamma=GAMMA, bootstrap=3)
            OnPolicyBatches(twin, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS).prepare()
            _, want = _q_steps(twin, 2, n, "value")
            for a, b in zip(got, want):
                for w in range(2):
                    for k in ("params", "grads", "m", "v"):
                        assert _same(a[w][k], b[w][k]), (w, k)
        finally:
            twin.close()
    else:
        learner.set_q_target("value")


def test_targets_follow_the_networks_after_target_updates_and_an_actor_step(prepared):
    """Q steps and update_targets move the target images, a pathwise step moves the policy: a re-evaluation differs from the first
    one and equals that of a fresh handle on which the current policy and the current TARGET networks were installed."""
    c = prepared("ieee13-tanh40")
    env = c["env"]
    h = env.handle
    _install(c)
    first = _evaluate(env)
    ql = P.DeviceLearner(env, nets=("q1", "q2"), **HYPER, q_target="policy")
    pl = P.DeviceLearner(env, nets=("policy",), **HYPER, policy_loss="pathwise", alpha=ALPHA, bc_coef=2.5, pathwise_seed=11)
    for s in range(2):
        ql.step(h.onpolicy_batch(5, s, 0, 185))
    same = _evaluate(env)                            # (a learner's step does not make the evaluation stale; the targets have not moved)
    assert _same(same["td_target"], first["td_target"])
    ql.update_targets(0.5)
    moved_q = _evaluate(env)
    assert _same(moved_q["next_actions"], first["next_actions"]) and not np.array_equal(moved_q["q_next"][0], first["q_next"][0])
    pl.step(h.onpolicy_batch(5, 0, 0, 185))
    got = _evaluate(env)
    assert not np.array_equal(got["next_pre_head"], moved_q["next_pre_head"]) and not np.array_equal(got["td_target"], moved_q["td_target"])
    twin, d2 = _twin(c, pol=pl.policy(), qs=[ql.target_q(w) for w in range(2)])
    try:
        _assert_equal_evaluations(_evaluate(twin), d2, got, c["data"], c["B"])
    finally:
        twin.close()
    ql.set_q_target("value")
    _install(c)


# ---- refusals and non-interference ----------------------------------------------------------------------------------------------------

def test_every_refusal_and_the_valid_calls_afterwards(prepared):
    c = prepared("scal11-relu")
    feeder, B, T, ep = c["feeder"], c["B"], c["T"], c["ep"]
    want = None
    env = _env(feeder, B, ep)
    try:
        h = env.handle
        cfg = lambda **kw: _lib.q_next_config(**dict(dict(gamma=GAMMA, alpha=ALPHA, bootstrap_mask=3, seed=SEED, draw=DRAW), **kw))
        env.set_policy(c["pol"], stochastic=True)
        env.set_q(0, c["qs"][0])
        _refused(lambda: h.rollout_evaluate_q_next(cfg()), S, "no rollout")
        env.set_q(0, None)
        env.reset(seed=3)
        rollout_device(env, T, reset=False, actions=c["data"]["actions"])
        _refused(lambda: h.rollout_evaluate_q_next(cfg()), S, "before gs_q_mlp_set")
        _refused(lambda: h.rollout_q_next_arrays(), S, "gs_rollout_evaluate_q_next has not run")
        _refused(lambda: h.rollout_q_next_download(), S, "gs_rollout_evaluate_q_next has not run")
        for w in range(2):
            env.set_q(w, c["qs"][w])
        f64 = P.MLPPolicy([c["pol"].weight0] + c["pol"].weights[1:], [c["pol"].bias0] + c["pol"].biases[1:], activation=c["pol"].activation,
                          head="gaussian_tanh", compute="float64")
        env.set_policy(f64, stochastic=True)
        _refused(lambda: h.rollout_evaluate_q_next(cfg()), S, "GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH")
        D, A = env.obs_dim, env.action_dim
        plain = P.MLPPolicy(*_layers([D, 64, A], 1), activation="relu", head="tanh", compute="float32")
        env.set_policy(plain)
        _refused(lambda: h.rollout_evaluate_q_next(cfg()), S, "GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH")
        env.set_policy(c["pol"], stochastic=True)
        for bad, text in ((cfg(struct_size=60), "struct_size"), (cfg(bootstrap_mask=4), "mask"), (cfg(bootstrap_mask=-1), "mask"), (cfg(gamma=math.nan), "gamma"),
                          (cfg(gamma=math.inf), "gamma"), (cfg(alpha=math.nan), "alpha"), (cfg(alpha=-0.5), "alpha"), (cfg(alpha=math.inf), "alpha")):
            _refused(lambda: h.rollout_evaluate_q_next(bad), I, text)
        two = cfg()
        two.stochastic = 2
        _refused(lambda: h.rollout_evaluate_q_next(two), I, "stochastic")
        _refused(lambda: h.q_set_target_source(2), I, "unknown source")
        _refused(lambda: h.q_set_target_source(-1), I, "unknown source")
        assert h.q_get_target_source() == "value"
        _refused(lambda: h.rollout_q_next_arrays(), S, "gs_rollout_evaluate_q_next has not run")
        # a Q step under POLICY without a current evaluation; under VALUE without gs_rollout_evaluate_q
        env.set_value(c["val"])
        P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
        OnPolicyBatches(env, B * T, policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS).prepare()
        learner = P.DeviceLearner(env, nets=("q1",), **HYPER, q_target="policy")
        batch = h.onpolicy_batch(5, 0, 0, 33)
        _refused(lambda: learner.step(batch), S, "gs_rollout_evaluate_q_next has not run")
        learner.set_q_target("value")
        _refused(lambda: learner.step(batch), S, "gs_rollout_evaluate_q has not run")
        learner.set_q_target("policy")
        assert learner.info("q1")["step"] == 0
        # after the refusals the valid calls give their bits
        got = _evaluate(env)
        learner.step(batch)
        assert learner.info("q1")["step"] == 1
        step = learner.download("q1", ("params",))["params"]
        env.set_policy(c["pol"], stochastic=True)      # installing a policy or a Q network makes the evaluation stale
        _refused(lambda: h.rollout_q_next_arrays(), S, "gs_rollout_evaluate_q_next has not run")
        _evaluate(env)
        env.set_q(1, c["qs"][1])
        _refused(lambda: h.rollout_q_next_download(), S, "gs_rollout_evaluate_q_next has not run")
        again = _evaluate(env)
        # the views after a further rollout
        rollout_device(env, T, reset=False, actions=c["data"]["actions"])
        _refused(lambda: h.rollout_q_next_arrays(), S, "gs_rollout_evaluate_q_next has not run")
        _refused(lambda: h.rollout_q_next_download(), S, "gs_rollout_evaluate_q_next has not run")
        want = (got, again, step, _rollout_arrays(env))
    finally:
        env.close()
    # the same calls on a handle that was never refused
    env, d = _twin(c)
    try:
        clean = _evaluate(env)
        for ref in want[:2]:
            _assert_equal_evaluations(clean, d, ref, want[3], B)
        env.set_q(0, c["qs"][0])
        P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
        OnPolicyBatches(env, B * T, policy=c["pol"], adv_norm="none", seed=5, fields=FIELDS).prepare()
        _evaluate(env)
        learner = P.DeviceLearner(env, nets=("q1",), **HYPER, q_target="policy")
        learner.step(env.handle.onpolicy_batch(5, 0, 0, 33))
        assert _same(learner.download("q1", ("params",))["params"], want[2])
    finally:
        env.close()


def test_a_handle_that_ran_the_new_evaluation_computes_what_it_computed_before(prepared):
    """Non-interference: the same rollout, gs_rollout_evaluate and gs_rollout_evaluate_q bits with and without the new entry."""
    c = prepared("ieee13-elu")
    T = c["T"]
    out = []
    for use in (False, True):
        env = _env(c["feeder"], c["B"], c["ep"])
        try:
            _install(dict(c, env=env))
            env.reset(seed=3)
            rollout_device(env, T, seed=7, reset=False)
            if use:
                _evaluate(env)
                env.handle.q_set_target_source("policy")
            P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
            P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
            if use:
                _evaluate(env, mask=1, stochastic=False)
            first = dict(_rollout_arrays(env), **env.handle.rollout_onpolicy_download(("values", "terminal_values", "advantages", "returns")))
            q = env.handle.rollout_q_download()
            rollout_device(env, T, seed=8, reset=False)
            second = _rollout_arrays(env)
            out.append((first, q, second))
        finally:
            env.close()
    (fa, qa, sa), (fb, qb, sb) = out
    for a, b in ((fa, fb), (sa, sb)):
        # (the terminal list is appended in no particular order: entry by entry through (t, b))
        oa, ob = (np.lexsort((d["terminal_index"][:, 1], d["terminal_index"][:, 0])) for d in (a, b))
        for k in a:
            if not isinstance(a[k], np.ndarray):               # (n_terminal)
                assert a[k] == b[k], k
                continue
            x, y = (a[k][oa], b[k][ob]) if k.startswith("terminal_") else (a[k], b[k])
            assert _same(x, y), k
    assert _same(fa["observations"], c["data"]["observations"])
    for src in ("online", "target"):
        assert _same(qa["q_min"][src], qb["q_min"][src])
        for w in range(2):
            assert _same(qa["q"][src][w], qb["q"][src][w])
    assert _same(qa["q_adv"], qb["q_adv"]) and _same(qa["td_target"], qb["td_target"])
