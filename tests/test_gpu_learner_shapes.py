"""GPU: the training kernels on non-square, shallow and deep networks -- the table of tests/learner_cases.py (held to its rules on the
host by tests/test_learner_cases_static.py) through ``gs_learner_step``, ``gs_rollout_evaluate_q`` and ``gs_learner_step_pathwise``,
against the NumPy restatements of grid_fed_rl_gym_amd.  What the square shapes of tests/test_gpu_learner.py, test_gpu_q_critics.py and
test_gpu_pathwise.py cannot see: the transposed image with kb != nt, depths 1 .. 4, tile counts 1 .. 16 with unequal ownership, the
weight-gradient kernel's half-empty output and partial input blocks, twins that differ from each other and from the policy.

Set-up as tests/test_gpu_learner.py: ``episode_length`` 7, a stochastic float32 policy, the reward critic and cost critics on
voltage and thermal, the normalisation from a short random rollout; ONE environment per feeder (13-bus B = 37, 123-bus B = 70), on
which every row installs its networks, resets, rolls out (T = 5; 14 for the row with n = 513; 123-bus 3), evaluates and prepares.
The twin rows collect a random-action rollout, so that cases A and B hold the same data.

Bounds are those files', none computed from the device: 4 E_ref per tensor (E_ref = the float32 restatement's error against
``exact=True``), the 1e-4 band around 1 +- clip with at most 2 % of a minibatch inside, the ``_mean_bound`` / fsum statistics rules,
Adam, images and noise-fed heads bit for bit.  One amendment, tests/test_gpu_learner.py's for the critic's last bias generalised: a
tensor of fewer than 32 entries (the pool ``_single_rows`` uses) has an E_ref that is a draw, not a statistic, so its E_ref is at
least 2^-24 max_entries sum_i |term_i| -- what rounding the n terms of an entry's sum to float32 can cost ANY evaluation of it; the
terms (delta_l[i][j] for db_l, delta_l[i][j] a_{l-1}[i][k] for dW_l) come from the exact restatement's ``backprop``."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd.learner import _pathwise_head, _pathwise_sample, adam_np, pathwise_grad_np, pathwise_noise_np, ppo_grad_np, value_grad_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, q_rollout_np, rollout_device
from tests import learner_cases as C
from tests import test_gpu_learner as TL

pytestmark = pytest.mark.gpu

CHANNELS = TL.CHANNELS
NETS = TL.NETS
CLIP, ENT, HYPER = TL.CLIP, TL.ENT, TL.HYPER
GAMMA = 0.97
ACTOR = dict(alpha=0.2, bc_coef=0.5, pathwise_seed=0x5EED0123456789)
FIELDS = ["observations", "actions", "advantages", "returns", "values", "indices"]
SMALL = 32                       # tensors with fewer entries take the floor
WORST = {}
FLOORED = set()
MISSED = []
_ENVS = {}
_STATE = {}                      # feeder: the key of what its environment holds prepared
_RECORDS = {}                    # twin case: its pathwise steps' q and dQ/da per twin


def _env(feeder):
    if feeder not in _ENVS:
        _ENVS[feeder] = TL._env(feeder, C.ROLLOUT[feeder][0])
    return _ENVS[feeder]


@pytest.fixture(scope="module", autouse=True)
def _environments():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    _STATE.clear()
    _RECORDS.clear()
    print("largest device error / E_ref:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("tensors that took the small-tensor floor:", sorted(FLOORED))


def _err(a, b):
    return TL._err(a, b)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _floors(exact):
    """{(kind, l): 2^-24 max_entries sum_i |term_i|} for the tensors of ``exact``'s gradient with fewer than SMALL entries"""
    bp, out = exact["backprop"], {}
    for l, (dW, db) in enumerate(exact["grads"]):
        d, a = np.abs(bp["deltas"][l]), np.abs(bp["acts"][l])
        if db.size < SMALL:
            out["db", l] = 2.0 ** -24 * float(np.max(d.sum(axis=0)))
        if dW.size < SMALL:
            out["dW", l] = 2.0 ** -24 * float(np.max(d.T @ a))
    return out


def _within(tag, what, got, exact, f32, floor=None):
    """tests/test_gpu_learner.py's ``_within`` (4 E_ref; every tensor is looked at before the test fails) with the floor of this
    file's docstring; both values of a floored tensor are printed"""
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    if floor is not None:
        print(f"{tag} {what}: E_ref {e_ref:.3e}, the float32 rounding of its terms {floor:.3e}")
        if floor > e_ref:
            FLOORED.add(what)
        e_ref = max(e_ref, floor)
    ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    key = what.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio if math.isfinite(ratio) else 1e9)
    if not e_dev <= 4.0 * e_ref:
        MISSED.append((tag, what, e_dev, e_ref))


def _gradient_within(tag, net, got, exact, f32):
    gW, gb = got
    floors = _floors(exact)
    for l in range(len(gW)):
        _within(tag, f"{net} dW[{l}]", gW[l], exact["grads"][l][0], f32["grads"][l][0], floors.get(("dW", l)))
        _within(tag, f"{net} db[{l}]", gb[l], exact["grads"][l][1], f32["grads"][l][1], floors.get(("db", l)))


def _adam_bit_for_bit(tag, learner, net, state, t):
    g = learner.download(net, ("grads",))["grads"]
    st = learner.stats(net)
    assert st["step"] == t, tag
    p, m, v = adam_np(state["params"], g, state["m"], state["v"], t, HYPER, st["grad_norm"])
    got = learner.download(net)
    assert np.array_equal(got["params"], p) and np.array_equal(got["m"], m) and np.array_equal(got["v"], v), (tag, net, t)
    return got


# ---- policy and critic steps --------------------------------------------------------------------------------------------------------

def _prepare_row(row):
    """the row's networks installed on the feeder's environment, its rollout collected, evaluated and prepared"""
    env = _env(row.feeder)
    key = ("row", C.row_id(row))
    B, T = C.SEGMENT_ROLLOUT if 513 in row.sizes else C.ROLLOUT[row.feeder]
    if _STATE.get(row.feeder, (None,))[0] == key:
        return _STATE[row.feeder][1]
    mean, std = TL._normalisation(row.feeder)
    pol = P.MLPPolicy(*C.draw(C.policy_dims(row.feeder, row.hidden), C.SEEDS["policy"]), activation=row.activation, head="gaussian_tanh", obs_mean=mean,
                      obs_std=std, compute="float32")
    vals = {name: P.MLPValue(*C.draw(C.value_dims(row.feeder, row.hidden), C.SEEDS[name]), activation=row.activation, obs_mean=mean, obs_std=std)
            for name in ("value", "voltage", "thermal")}
    c = dict(env=env, pol=pol, vals=vals, feeder=row.feeder, B=B, T=T, activation=row.activation)
    TL._install(c)
    env.reset(seed=3)
    rollout_device(env, T, seed=7, reset=False, policy=True)
    P.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
    P.rollout_costs(env, P.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5), kinds="excess")
    P.evaluate_rollout_costs(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
    c["batches"] = OnPolicyBatches(env, min(B * T, 4096), policy=pol, adv_norm="rollout", seed=5,
                                   fields=["observations", "actions", "log_probs", "advantages", "returns", "values", "indices", "cost_returns"])
    c["batches"].prepare()
    h = env.handle
    c["actions"] = h.rollout_download(want=("actions",))["actions"].reshape(B * T, -1)
    c["logp"] = h.rollout_onpolicy_download(("log_probs",))["log_probs"].reshape(B * T)
    _STATE[row.feeder] = (key, c)
    return c


def _check_policy_step(tag, c, learner, hb, params, n):
    """tests/test_gpu_learner.py's ``_check_policy_step`` (n >= 32) with the small-tensor floor"""
    idx = hb["indices"]
    act, lp_old = c["actions"][idx], c["logp"][idx]
    views = {k: v.to_host() for k, v in learner.views("policy").items()}
    dev_flags = views["clipped"]
    layers = TL._pairs(*params)
    kw = dict(activation=c["activation"])
    exact = ppo_grad_np(layers, hb["observations"], act, lp_old, hb["advantages"], CLIP, ENT, exact=True, clipped=dev_flags, **kw)
    f32 = ppo_grad_np(layers, hb["observations"], act, lp_old, hb["advantages"], CLIP, ENT, exact=False, clipped=dev_flags, **kw)
    r = exact["ratio"]
    band = (np.abs(r - (1.0 + CLIP)) <= 1e-4 * (1.0 + CLIP)) | (np.abs(r - (1.0 - CLIP)) <= 1e-4 * (1.0 - CLIP))
    assert band.sum() <= 0.02 * n, (tag, int(band.sum()))
    assert np.array_equal(dev_flags[~band], exact["clipped"][~band]), tag
    print(f"{tag}: clipped {int(dev_flags.sum())} of {n}, in the band {int(band.sum())}, log_std outside the clamp {int(exact['log_std_outside'].sum())}")
    _gradient_within(tag, "policy", learner.gradients("policy"), exact, f32)
    _within(tag, "log_probs_new", views["log_probs_new"], exact["log_probs_new"], f32["log_probs_new"])
    assert np.allclose(views["ratio"], np.exp(views["log_probs_new"] - lp_old), rtol=1e-15, atol=0.0), tag
    st = learner.stats("policy")
    adv = hb["advantages"].astype(np.float64)
    surr_terms = np.minimum(views["ratio"] * adv, np.clip(views["ratio"], 1.0 - CLIP, 1.0 + CLIP) * adv)
    assert np.array_equal(views["loss_terms"], surr_terms), tag
    surr, ent = math.fsum(surr_terms) / n, math.fsum(views["entropy_terms"]) / n
    kl_terms = lp_old - views["log_probs_new"]
    b_surr, b_ent, b_kl = TL._mean_bound(surr_terms, n), TL._mean_bound(views["entropy_terms"], n), TL._mean_bound(kl_terms, n)
    assert abs(st["surrogate"] - surr) <= b_surr and abs(st["entropy"] - ent) <= b_ent, (tag, st, surr, ent)
    assert abs(st["approx_kl"] - math.fsum(kl_terms) / n) <= b_kl, (tag, st)
    assert abs(st["loss"] - (-surr - ENT * ent)) <= b_surr + ENT * b_ent + 4 * TL.U * (abs(surr) + ENT * abs(ent)), (tag, st)
    assert st["clip_fraction"] == int(dev_flags.sum()) / n and math.isnan(st["value_loss"]), (tag, st)
    flat = learner.download("policy", ("grads",))["grads"]
    norm = math.sqrt(math.fsum(float(x) * float(x) for x in flat))
    assert abs(st["grad_norm"] - norm) <= flat.size * 2.0 ** -52 * norm, (tag, st["grad_norm"], norm)
    return int(dev_flags.sum())


def _check_value_step(tag, c, learner, net, hb, params, n):
    """tests/test_gpu_learner.py's ``_check_value_step`` (n >= 32); its floor for the last bias is the small-tensor floor of db[last]"""
    ret = hb["returns"] if net == "value" else hb["cost_returns"][CHANNELS[net]]
    layers = TL._pairs(*params)
    exact = value_grad_np(layers, hb["observations"], ret, exact=True, activation=c["activation"])
    f32 = value_grad_np(layers, hb["observations"], ret, exact=False, activation=c["activation"])
    last = len(layers) - 1
    assert math.isclose(_floors(exact)["db", last], 2.0 ** -24 * math.fsum(np.abs(2.0 * (exact["values"] - ret.astype(np.float64)) / n)), rel_tol=1e-12)
    _gradient_within(tag, net, learner.gradients(net), exact, f32)
    views = learner.views(net)
    assert views["log_probs_new"] is None and views["ratio"] is None and views["clipped"] is None
    terms = views["loss_terms"].to_host()
    st = learner.stats(net)
    assert abs(st["value_loss"] - math.fsum(terms) / n) <= TL._mean_bound(terms, n) and st["loss"] == st["value_loss"], (tag, st)
    assert all(math.isnan(st[k]) for k in ("surrogate", "entropy", "approx_kl", "clip_fraction"))
    flat = learner.download(net, ("grads",))["grads"]
    norm = math.sqrt(math.fsum(float(x) * float(x) for x in flat))
    assert abs(st["grad_norm"] - norm) <= flat.size * 2.0 ** -52 * norm, (tag, st["grad_norm"], norm)


ALL = [(row, n) for row in C.TABLE for n in row.sizes]


@pytest.mark.parametrize("row,n", ALL, ids=[f"{C.row_id(r)}-n{n}" for r, n in ALL])
def test_three_steps_against_the_restatements(row, n):
    """tests/test_gpu_learner.py's test of the same name on every row of the table: gradients, flags, per-sample arrays and
    statistics at freshly created parameters and after two steps (step 3 reads the transposed image Adam rewrote twice); Adam's
    parameters and moments bit for bit over the three steps, weight decay and the norm clip on.

    Observed on the MI355X (17 cases, device error / E_ref, largest per kind): policy dW 3.12 (dW[3] of (17, 240, 1) at n = 33, six
    entries), db 2.80, log_probs_new 2.52; reward critic dW 1.83, db 1.85; thermal cost critic dW 2.10, db 3.79 (the one-entry db[3]
    of (200, 24, 136) at n = 185 under its floor: E_ref 1.83e-8, floor 1.88e-8, device 7.1e-8).  The floor was the larger of the two
    values for: policy db[0] .. db[3]; reward critic dW[1], dW[3], db[0] .. db[3]; thermal critic dW[1], db[0] .. db[3] -- each only
    in the rows where that tensor has fewer than 32 entries."""
    c = _prepare_row(row)
    h = c["env"].handle
    TL._install(c)
    MISSED.clear()
    learner = P.DeviceLearner(c["env"], nets=NETS, **HYPER)
    f = C.facts(C.policy_dims(row.feeder, row.hidden), n)
    info = learner.info("policy")
    assert info["rows_per_segment"] == C.GS_TR_SEG and info["param_count"] == f["P"] and list(info["dims"]) == C.policy_dims(row.feeder, row.hidden)
    state = {net: learner.download(net) for net in NETS}
    clipped = 0
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = TL._host(batch)
        params = {net: learner.parameters(net) for net in NETS}
        learner.step(batch)
        if s in (0, 2):
            tag = f"{C.row_id(row)} n={n} step {s + 1}"
            clipped += _check_policy_step(tag, c, learner, hb, params["policy"], n)
            for net in ("value", "thermal"):
                _check_value_step(tag, c, learner, net, hb, params[net], n)
        for net in NETS:
            state[net] = _adam_bit_for_bit((C.row_id(row), n), learner, net, state[net], s + 1)
    assert not MISSED, MISSED


@pytest.mark.parametrize("hidden", [(96, 40), (256, 17, 256)], ids=["96x40", "256x17x256"])
def test_the_refreshed_images_are_the_parameters(hidden):
    """tests/test_gpu_learner.py's twin-handle check: after three steps the rollout and critic kernels read what
    ``set_policy(learner.policy())`` would have installed on a fresh handle -- padding too"""
    row = next(r for r in C.TABLE if r.hidden == hidden)
    c = _prepare_row(row)
    env = c["env"]
    learner = TL._three_steps(c)
    twin = TL._env(row.feeder, C.ROLLOUT[row.feeder][0])
    try:
        twin.set_policy(learner.policy(), stochastic=True)
        twin.set_value(learner.value("value"))
        twin.set_cost_value("thermal", learner.value("thermal"))
        twin.set_cost_value("voltage", c["vals"]["voltage"])
        out = []
        for e in (env, twin):
            e.reset(seed=21)
            a = e.policy_actions(seed=9, t=2)
            rollout_device(e, 5, seed=13, reset=False, policy=True)
            P.evaluate_rollout(e, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
            P.rollout_costs(e, P.ConstraintLimits.of(e, voltage=(0.97, 1.03), thermal=0.5), kinds="excess")
            P.evaluate_rollout_costs(e, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
            d = e.handle.rollout_download(want=("observations", "actions", "rewards"))
            o = e.handle.rollout_onpolicy_download(("log_probs", "values", "advantages"))
            cd = e.handle.rollout_costs_download(("values",), channels=(2,))
            out.append(dict(a=a, cost_values=cd["values"][2], **d, **o))
    finally:
        twin.close()
        _STATE.pop(row.feeder, None)           # the environment's rollout was replaced
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert not np.array_equal(learner.parameters("policy")[0][0], c["pol"].weight0.astype(np.float32))      # it did learn


# ---- the twins ----------------------------------------------------------------------------------------------------------------------

def _q_net(case, hidden, mean, std):
    D = C.WIDTHS[case.feeder][0]
    return None if hidden is None else P.MLPQ(*C.draw(C.q_dims(case.feeder, hidden), C.q_seed(hidden)), D, activation=case.q_activation, obs_mean=mean, obs_std=std)


def _install_twins(c):
    env = c["env"]
    env.set_policy(c["pol"], stochastic=True)
    env.set_value(c["val"])
    for w in range(2):
        env.set_q(w, c["qs"][w])


def _evaluate_q(env):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    return P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)


def _prepare_twins(case):
    """the case's policy and twins installed, a random-action rollout collected (the same for every case of a feeder), evaluated and
    the minibatches prepared"""
    env = _env(case.feeder)
    key = ("twins", case.name)
    if _STATE.get(case.feeder, (None,))[0] == key:
        c = _STATE[case.feeder][1]
        _install_twins(c)
        return c
    B, T = C.ROLLOUT[case.feeder]
    mean, std = TL._normalisation(case.feeder)
    pol = P.MLPPolicy(*C.draw(C.policy_dims(case.feeder, case.policy), C.SEEDS["policy"]), activation=case.policy_activation, head="gaussian_tanh",
                      obs_mean=mean, obs_std=std, compute="float32")
    val = P.MLPValue(*C.draw(C.value_dims(case.feeder, (64,)), C.SEEDS["value"]), activation="relu", obs_mean=mean, obs_std=std)
    qs = [_q_net(case, q, mean, std) for q in (case.q1, case.q2)]
    c = dict(env=env, pol=pol, val=val, qs=qs, installed=tuple(w for w in range(2) if qs[w] is not None), feeder=case.feeder, B=B, T=T, case=case)
    _install_twins(c)
    env.reset(seed=3)
    rollout_device(env, T, seed=7, reset=False)
    c["data"] = env.handle.rollout_download(want=("observations", "actions", "rewards", "terminals"))
    _evaluate_q(env)
    OnPolicyBatches(env, B * T, policy=pol, adv_norm="none", seed=5, fields=FIELDS).prepare()
    _STATE[case.feeder] = (key, c)
    return c


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_q_of_every_stored_pair_and_of_a_row_in_another_batch(name):
    """tests/test_gpu_q_critics.py's rule and margin for gs_k_q_mlp_f32 on twins of different shapes (E: a linear twin whose dot
    product runs over three input panels), and a row's value on a handle of another B, bit for bit.

    Observed on the MI355X: device error / E_ref at most 1.86 over the six twins."""
    case = C.TWIN_CASES[name]
    c = _prepare_twins(case)
    env, d = c["env"], c["data"]
    out = _evaluate_q(env)
    assert out.installed == (0, 1) and out.rows_per_tile == 64
    got = env.handle.rollout_q_download(("q",))["q"]
    for w in range(2):
        exact = q_rollout_np(c["qs"][w], d["observations"], d["actions"], exact=True)
        e_ref = _err(q_rollout_np(c["qs"][w], d["observations"], d["actions"]), exact)
        err = _err(got["online"][w], exact)
        print(f"{name} twin {w}: E_ref {e_ref:.3e} max |device - exact| {err:.3e} ratio {err / e_ref:.2f}")
        WORST["q forward"] = max(WORST.get("q forward", 0.0), err / e_ref)
        assert e_ref > 0.0 and err <= 4.0 * e_ref, (w, err, e_ref)
        assert np.std(exact) > 1e-3
        assert _same(got["online"][w], got["target"][w]), "the target image is a copy of the online image"
    assert not np.array_equal(got["online"][0], got["online"][1])
    # the first B2 instances on a handle of B2: other tiles, the same bits
    B2 = 7 if case.feeder == "ieee13" else 37
    twin = TL._env(case.feeder, B2)
    try:
        _install_twins(dict(c, env=twin))
        twin.reset(seed=3)
        rollout_device(twin, c["T"], reset=False, actions=np.ascontiguousarray(d["actions"][:, :B2]))
        assert _same(twin.handle.rollout_download(want=("observations",))["observations"], np.ascontiguousarray(d["observations"][:, :B2]))
        _evaluate_q(twin)
        other = twin.handle.rollout_q_download(("q",))["q"]
        for w in range(2):
            assert _same(np.ascontiguousarray(got["online"][w][:, :B2]), other["online"][w]), w
    finally:
        twin.close()


def _sa(c, hb):
    act = c["data"]["actions"].reshape(c["B"] * c["T"], -1)[hb["indices"]]
    return np.concatenate([hb["observations"], act.astype(np.float32)], axis=1)


@pytest.mark.parametrize("name", ["A", "C"])
def test_three_q_steps_against_the_restatements(name):
    """tests/test_gpu_q_critics.py's test of the same name on twins of different shapes: both regress on float32(td_target[idx]) over
    [obs | float32(act)]; gradients at fresh parameters and after two steps, Adam bit for bit; then the trained networks evaluate
    the rollout as a second handle does on which ``learner.q(k)`` was installed.

    Observed on the MI355X: dW at most 1.24, db 1.00; the floor was the larger value for db[0] (the linear twin), db[1] and db[3]
    (last biases)."""
    case = C.TWIN_CASES[name]
    c = _prepare_twins(case)
    env = c["env"]
    h = env.handle
    _evaluate_q(env)
    td = h.rollout_q_download(("td_target",))["td_target"].reshape(-1)
    MISSED.clear()
    nets = ("q1", "q2")
    n = 185
    learner = P.DeviceLearner(env, nets=nets, **HYPER)
    for w, net in enumerate(nets):
        assert learner.info(net)["param_count"] == C.q_facts(case.feeder, (case.q1, case.q2)[w])["P"]
    state = {net: learner.download(net) for net in nets}
    kw = dict(activation=case.q_activation)
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = {k: v.to_host() for k, v in batch.items() if v is not None and not isinstance(v, list)}
        sa, y = _sa(c, hb), td[hb["indices"]].astype(np.float32)
        params = {net: learner.parameters(net) for net in nets}
        learner.step(batch)
        for net in nets:
            tag = f"{name} n={n} step {s + 1} {net}"
            if s in (0, 2):
                layers = list(zip(*params[net]))
                exact, f32 = value_grad_np(layers, sa, y, exact=True, **kw), value_grad_np(layers, sa, y, exact=False, **kw)
                _gradient_within(tag, "q", learner.gradients(net), exact, f32)
            st = learner.stats(net)
            assert st["loss"] == st["value_loss"]
            state[net] = _adam_bit_for_bit(tag, learner, net, state[net], s + 1)
    assert not MISSED, MISSED
    _evaluate_q(env)
    got = h.rollout_q_download(("q",))["q"]
    trained = [learner.q(w) for w in range(2)]
    twin = TL._env(case.feeder, c["B"])
    try:
        _install_twins(dict(c, env=twin, qs=trained))
        twin.reset(seed=3)
        rollout_device(twin, c["T"], reset=False, actions=c["data"]["actions"])
        assert _same(twin.handle.rollout_download(want=("observations",))["observations"], c["data"]["observations"])
        _evaluate_q(twin)
        want = twin.handle.rollout_q_download(("q",))["q"]
        for w in range(2):
            assert _same(got["online"][w], want["online"][w]), w
            assert not np.array_equal(got["online"][w], got["target"][w])
    finally:
        twin.close()
        _install_twins(c)


def _views(learner):
    v = learner.pathwise_views()
    n, A = v["actions"].shape
    out = {k: x.to_host() for k, x in v.items() if hasattr(x, "to_host")}
    flat, stride = out.pop("pre_head"), v["pre_head_stride"]
    out["pre_head"] = np.stack([flat[i * stride:i * stride + 2 * A] for i in range(n)])
    for k in ("q", "dq_da"):
        out[k] = [None if x is None else x.to_host() for x in v[k]]
    out["installed"] = tuple(v["installed"])
    return out


def _actor_steps(name, n=185):
    """three pathwise steps of case ``name`` with tests/test_gpu_pathwise.py's checks; returns per step the twins' q and dQ/da"""
    if name in _RECORDS:
        return _RECORDS[name]
    case = C.TWIN_CASES[name]
    c = _prepare_twins(case)
    env = c["env"]
    h = env.handle
    D, A = C.WIDTHS[case.feeder]
    installed = c["installed"]
    hiddens = (case.q1, case.q2)
    _evaluate_q(env)
    before = h.rollout_q_download(("q",))["q"] if len(installed) == 2 else None
    tw = tuple(f"q{w + 1}" for w in installed)
    ql = P.DeviceLearner(env, nets=tw, **HYPER)
    learner = P.DeviceLearner(env, nets=("policy",), **HYPER, policy_loss="pathwise", **ACTOR)
    assert learner.loss("policy")["name"] == "pathwise" and learner.info("policy")["dims"][-1] == 2 * A
    q_layers = [list(zip(*ql.parameters(net))) for net in tw]
    q_state = {net: ql.download(net) for net in tw}
    state = learner.download("policy")
    stored_all = c["data"]["actions"].reshape(c["B"] * c["T"], -1)
    kw = dict(activation=case.policy_activation, q_activation=case.q_activation)
    records = []
    for s in range(3):
        batch = h.onpolicy_batch(5, s, 0, n)
        hb = {k: v.to_host() for k, v in batch.items() if v is not None and not isinstance(v, list)}
        stored = stored_all[hb["indices"]]
        layers = list(zip(*learner.parameters("policy")))
        learner.step(batch)
        v = _views(learner)
        tag = f"{name} n={n} step {s + 1}"
        assert v["installed"] == installed, tag
        # the noise, and the heads fed what the device's heads read
        e_noise = _err(v["noise"], pathwise_noise_np(ACTOR["pathwise_seed"], s, n, A))
        print(f"{tag} noise: max |device - pathwise_noise_np| {e_noise:.3e}")
        assert e_noise <= 1e-9 and np.std(v["noise"]) > 0.1
        inside, std, eps, a, lp = _pathwise_sample(v["pre_head"].astype(np.float64), v["noise"])
        assert _same(v["actions"], a) and _same(v["log_probs"], lp), tag
        listed = np.array([installed.index(w) for w in v["which"]])       # the device's choices as positions among the installed twins
        found, use, qmin, bc, terms, ghead = _pathwise_head(inside, std, eps, a, lp, [v["q"][w] for w in installed], [v["dq_da"][w] for w in installed],
                                                            ACTOR["alpha"], ACTOR["bc_coef"], stored, False)
        assert np.array_equal(listed, found) and _same(v["q_min"], qmin) and _same(v["bc_terms"], bc) and _same(v["loss_terms"], terms), tag
        for w in range(2):
            if w not in installed:
                assert v["q"][w] is None and v["dq_da"][w] is None
        # q and dQ/da per twin, the policy's gradient
        if s in (0, 2):
            exact = pathwise_grad_np(layers, q_layers, hb["observations"], v["noise"], ACTOR["alpha"], ACTOR["bc_coef"], stored_actions=stored, exact=True, which=listed, **kw)
            f32 = pathwise_grad_np(layers, q_layers, hb["observations"], v["noise"], ACTOR["alpha"], ACTOR["bc_coef"], stored_actions=stored, exact=False, which=listed, **kw)
            for j, w in enumerate(installed):
                _within(tag, f"q[{w}]", v["q"][w], exact["q"][j], f32["q"][j])
                if hiddens[w]:
                    _within(tag, f"dq_da[{w}]", v["dq_da"][w], exact["dq_da"][j], f32["dq_da"][j])
            _gradient_within(tag, "actor", learner.gradients("policy"), exact, f32)
            assert np.std(exact["q"]) > 1e-3 and all(np.abs(g).max() > 0.0 for g in learner.gradients("policy")[0])
        for j, w in enumerate(installed):          # a linear twin: the action columns of W0 bit for bit
            if not hiddens[w]:
                w0 = q_layers[j][0][0].astype(np.float32)
                assert _same(v["dq_da"][w], np.ascontiguousarray(np.broadcast_to(w0[0, D:], (n, A)))), (tag, w)
        st = learner.stats("policy")
        assert math.isnan(st["approx_kl"]) and math.isnan(st["clip_fraction"]) and math.isnan(st["value_loss"])
        assert math.isclose(st["loss"], math.fsum(v["loss_terms"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        assert math.isclose(st["surrogate"], math.fsum(v["q_min"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        assert math.isclose(st["entropy"], -math.fsum(v["log_probs"]) / n, rel_tol=1e-12, abs_tol=1e-300)
        state = _adam_bit_for_bit(tag, learner, "policy", state, s + 1)
        records.append({w: (v["q"][w], v["dq_da"][w]) for w in installed})
    # the twins were read, not written: their parameters, and the images the evaluation reads
    for net in tw:
        now = ql.download(net)
        assert all(_same(now[k], q_state[net][k]) for k in now) and ql.info(net)["step"] == 0, net
    if before is not None:
        _evaluate_q(env)
        after = h.rollout_q_download(("q",))["q"]
        for src in ("online", "target"):
            assert all(_same(after[src][w], before[src][w]) for w in range(2)), src
    _RECORDS[name] = records
    return records


@pytest.mark.parametrize("name", [t.name for t in C.TWINS])
def test_three_actor_steps_against_the_restatements(name):
    """tests/test_gpu_pathwise.py's checks on policies and twins of different shapes and activations: noise and heads to the bit, q
    and dQ/da per twin and the policy's gradient under 4 E_ref (the device's choice of twin fed to both restatements), Adam bit for
    bit over three steps, the twins' parameters and images untouched.  Case B: twin k's q and dQ/da are bit-equal to what case A
    gave the same network at the other index -- neither twin reads what its sibling left in the shared scratch.

    Observed on the MI355X: q 1.24, dq_da 3.88 (case D, H0 = 200: ONE float32 chain of 200 products against a host matrix product
    that sums in blocks; 3.02 at step 3), the policy's dW 1.80, db 1.40; the floor was the larger value for db[0] (C, the linear
    policy's six biases; D, seventeen), db[2] (D, the one-unit layer) and db[3] (D, the head)."""
    MISSED.clear()
    records = _actor_steps(name)
    assert not MISSED, MISSED
    if name == "B":
        first = _actor_steps("A")
        assert not MISSED, MISSED
        for s in range(3):
            for w in range(2):
                assert _same(records[s][w][0], first[s][1 - w][0]) and _same(records[s][w][1], first[s][1 - w][1]), (s, w)
