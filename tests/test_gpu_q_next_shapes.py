"""GPU: the policy-action TD targets (``gs_k_policy_rows_f32``, ``gs_k_q_mlp_rows_f32``, ``gs_k_q_next_td``, the buffers of
abi_q_next.hip) at their tile, head and buffer edges -- the table of tests/q_next_cases.py, held to its rules on
the host by tests/test_q_next_cases_static.py.  What the square networks, the four datasets and the repeated rollouts of
tests/test_gpu_q_next.py cannot see:

(a) network shapes   every hidden shape of ``learner_cases.TABLE`` as the policy with twins of the same widths, and ``TWINS`` A to E,
                     on that file's 13-bus dataset (B = 5, T = 37: 185 rows) and, for E, its 123-bus one (T = 3, B = 70)
(b) head and staging A = 1, 2, 5, 7, 18 and D = 40, 82, 345, 320, 1193 on five synthetic feeders, hidden (64, 64) relu
(c) the extremes     two policies whose last biases put log_std beyond both clamp ends and the mean beyond gw_tanh's cap
(d) the tiles        1, 64, 65, 128 rows and 0, 32, 64, 65 list entries, as replays of a prefix of a 260-row rollout with 130
                     entries on fresh handles, every output of a row bit-equal to the larger evaluation's
(e) buffer reuse     a shorter rollout after a longer one on the same handle, and a longer one after a shorter one

The checks are those of ``test_policy_rows_target_twins_and_targets_against_the_restatements`` (``_check`` below, which takes an
empty terminal list, one twin alone and the deterministic head as well); the bounds are the project's, none computed from the device:
``*_pre_head`` and ``*_q`` within 4 E_ref of ``exact=True``, the noise within 1e-9 of ``q_next_noise_np``, actions and
log-probabilities bit-equal to ``policy_rows_np`` fed the device's pre-head values and noise, the minimum, ``term_value`` and
``td_target`` bit-equal to ``td_policy_np`` fed the device's arrays.

Row counts of the wide feeders of (b) come from section 25's yardstick (``q_next_cases.chain_yardstick``, host only: one ascending
float32 chain over 20 draws of N(0, 1) rows, its error over E_ref; at most 3.0 asked for): D = 345 and D = 320 give 1.00 at 162 and at
81 rows (NumPy's own product is such a chain at these widths), D = 1193 gives a median of 2.36 and at most 2.91 at 460 rows, 2.34 and
2.89 at 230 rows (B = 10, T = 46, ``episode_length`` 2 under limits only the time limit reaches).  At that width the largest of the 20
draws does not fall with the row count (between 2.7 and 3.9 from 90 to 780 rows, the median 2.1 to 2.5 throughout); 460 / 230 is the
smallest pair of the scan with both counts at or below 3.0."""
import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, policy_rows_np, q_next_noise_np, q_rollout_np, rollout_device, td_policy_np
from tests import learner_cases as L
from tests import q_next_cases as C
from tests import test_gpu_q_next as TQ

pytestmark = pytest.mark.gpu

GAMMA, ALPHA, SEED, DRAW = TQ.GAMMA, TQ.ALPHA, TQ.SEED, TQ.DRAW
ARRAYS = ("next_pre_head", "next_actions", "next_noise", "next_log_probs", "q_next_min", "td_target")
TERM_ARRAYS = ("term_pre_head", "term_actions", "term_noise", "term_log_probs", "term_q_min", "term_value")
WORST = {}
_SHARED = {}                    # dataset name / "base": the environment, its rollout's arrays and what was evaluated on it
_FRESH = {}                     # replay name: its rollout's arrays and evaluations, from a handle that is closed again
_NORM = {}
_same, _err = TQ._same, TQ._err


@pytest.fixture(scope="module", autouse=True)
def _environments():
    yield
    for c in _SHARED.values():
        c["env"].close()
    _SHARED.clear()
    _FRESH.clear()
    print("largest device error / E_ref:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def _env(feeder, B, episode_length, limits):
    fs = C.feeder(feeder)
    return P.BatchedGridEnvironment(fs, num_envs=B, solver=C.FEEDERS[feeder].solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=episode_length, voltage_limits=limits)


def _normalisation(feeder):
    """tests/test_gpu_q_next.py's ``_normalisation`` (its own cache for its feeders)"""
    if feeder in TQ.FEEDERS:
        return TQ._normalisation(feeder)
    if feeder not in _NORM:
        env = _env(feeder, 64, 7, (0.98, 1.02))
        try:
            obs = P.collect_random_data(env, 4, seed=11)["observations"]
        finally:
            env.close()
        mean, std = obs.mean(axis=0), obs.std(axis=0)
        constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
        _NORM[feeder] = (mean, np.where(constant, 1.0, std + 1e-6))
    return _NORM[feeder]


SQUARE_TWINS = ((C.SQUARE, 20), (C.SQUARE, 21))          # tests/test_gpu_q_next.py's twins


def _networks(feeder, policy=C.SQUARE, policy_activation="relu", twins=SQUARE_TWINS, q_activation="relu", bias=None):
    f = C.FEEDERS[feeder]
    mean, std = _normalisation(feeder)
    pol = P.MLPPolicy(*C.policy_layers(f.D, f.A, policy, bias), activation=policy_activation, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")
    qs = [None if t is None else P.MLPQ(*C.q_layers(f.D, f.A, t[0], t[1]), f.D, activation=q_activation, obs_mean=mean, obs_std=std) for t in twins]
    return pol, qs


def _install(env, pol, qs):
    env.set_policy(pol, stochastic=True)
    for w in range(2):
        env.set_q(w, qs[w])


def _collect(env, T, actions=None):
    """tests/test_gpu_q_next.py's collection: reset(seed=3), then T steps of random (seed 7) or of the uploaded actions"""
    env.reset(seed=3)
    if actions is None:
        rollout_device(env, T, seed=7, reset=False)
    else:
        rollout_device(env, T, reset=False, actions=np.ascontiguousarray(actions))
    return TQ._rollout_arrays(env)


def _close(tag, what, got, exact, f32):
    e_ref, e_dev = _err(f32, exact), _err(got, exact)
    ratio = e_dev / e_ref if e_ref > 0.0 else float("inf")
    print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f}")
    key = what.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), min(ratio, 1e9))
    assert e_ref > 0.0 and e_dev <= 4.0 * e_ref, (tag, what, e_dev, e_ref)


def _check(tag, env, d, pol, qs, stochastic=True, mask=3, inside=True):
    """The checks of tests/test_gpu_q_next.py's ``test_policy_rows_target_twins_and_targets_against_the_restatements`` on the
    evaluation of ``d``, the rollout ``env`` holds, under the installed ``pol`` and ``qs`` (None: that twin is not installed).  An
    empty terminal list has nothing to hold against E_ref and everything else to show: its arrays are there with length 0.
    ``inside``: the policy keeps its actions away from saturation.  Returns the download."""
    T, B = d["rewards"].shape
    D, A = env.obs_dim, env.action_dim
    installed = tuple(w for w in range(2) if qs[w] is not None)
    got = TQ._evaluate(env, mask, stochastic=stochastic)
    view = env.handle.rollout_q_next_arrays()
    n = len(d["terminal_index"])
    assert view["installed"] == installed and view["rows_per_tile"] == C.GS_VAL_ROWS and view["n_terminal"] == n
    assert view["next_pre_head"].shape == (T, B, 2 * A) and view["next_actions"].shape == (T, B, A) and view["term_value"].shape == (n,)
    assert got["term_pre_head"].shape == (n, 2 * A) and got["term_actions"].shape == (n, A) and got["term_value"].shape == (n,)
    for k in ARRAYS + TERM_ARRAYS:
        assert _same(view[k].to_host(), got[k]), k
    index = {"next": np.arange(T * B), "term": d["terminal_index"][:, 0].astype(np.int64) * B + d["terminal_index"][:, 1]}
    obs = {"next": d["next_observations"].reshape(T * B, D), "term": d["terminal_obs"].reshape(n, D)}
    for part, rows in (("next", T * B), ("term", n)):
        key = lambda k: f"{part}_{k}"
        pre = got[key("pre_head")].reshape(rows, 2 * A)
        act, eps, lp = got[key("actions")].reshape(rows, A), got[key("noise")].reshape(rows, A), got[key("log_probs")].reshape(rows)
        q = [(got["q_next"][w] if part == "next" else got["term_q"][w]).reshape(rows) for w in range(2)]
        for w in range(2):
            assert (view["q_next" if part == "next" else "term_q"][w] is not None) == (w in installed)
            if w not in installed:
                assert np.isnan(q[w]).all(), (part, w)
        if rows == 0:
            continue
        exact, f32 = policy_rows_np(pol, obs[part], None, exact=True)[0], policy_rows_np(pol, obs[part], None)[0]
        _close(tag, f"{part}_pre_head", pre, exact, f32)
        if stochastic:
            assert _err(eps, q_next_noise_np(SEED, DRAW, index[part], A, terminal=part == "term")) <= 1e-9 and np.std(eps) > 0.1
        else:
            assert not eps.any() and not np.signbit(eps).any()
        _, want_a, want_lp = policy_rows_np(pol, obs[part], eps, pre_head=pre)
        assert _same(act, want_a) and _same(lp, want_lp), (tag, part)
        assert np.isfinite(act).all() and np.isfinite(lp).all()
        if inside:
            assert np.std(act) > 1e-2 and (np.abs(act) < 1.0).all()
        for w in installed:
            o3, a3 = obs[part][None], act[None]
            _close(tag, f"{part}_q[{w}]", q[w], q_rollout_np(qs[w], o3, a3, exact=True)[0], q_rollout_np(qs[w], o3, a3)[0])
        want_min = np.fmin(q[0], q[1]) if len(installed) == 2 else q[installed[0]]
        assert _same(got["q_next_min" if part == "next" else "term_q_min"].reshape(rows), want_min), (tag, part)
    if len(installed) == 2:
        assert not np.array_equal(got["q_next"][0], got["q_next"][1])
    assert _same(got["term_value"], got["term_q_min"] - ALPHA * got["term_log_probs"])
    assert _same(got["td_target"], TQ._td(d, got, mask, ALPHA)), tag
    if n == 0:
        assert _same(got["td_target"], td_policy_np(d["rewards"], got["next_log_probs"], got["q_next_min"], d["terminals"], [], np.zeros((0, 2)), GAMMA, ALPHA, mask))
    return got


# ---- (a) network shapes -------------------------------------------------------------------------------------------------------------

def _dataset(name):
    """the random-action rollout of tests/test_gpu_q_next.py on ``C.DATA[name]``, collected once: it does not depend on the networks"""
    if name not in _SHARED:
        data = C.DATA[name]
        env = _env(data.feeder, data.B, data.episode_length, data.limits)
        _SHARED[name] = dict(env=env, data=_collect(env, data.T))
    return _SHARED[name]


@pytest.mark.parametrize("name", [s.name for s in C.SHAPES])
def test_network_shapes_against_the_restatements(name):
    """Every layer of the policy kernel is gq_layer<4, FULL>, the padded last one too: narrow layers with idle wavefronts, a
    wavefront with two tiles, four layers, a one-unit layer, the rectangular pair; the Q kernel's second launch form under twins of
    different depth and row stride in both orders, a linear twin, one twin alone.

    Observed on the MI355X: see DESIGN.md section 25 "The edges"."""
    s = C.SHAPE_CASES[name]
    c = _dataset(s.data)
    env, d = c["env"], c["data"]
    f = C.FEEDERS[s.data]
    assert (env.obs_dim, env.action_dim) == (f.D, f.A) and d["rewards"].shape == (C.DATA[s.data].T, C.DATA[s.data].B)
    flags = d["terminals"]
    if s.data == "ieee13":
        assert (flags == 1).any() and ((flags & 2) != 0).any(), "the dataset ends episodes under both done bits"
    else:
        assert (flags != 0).sum() >= C.DATA[s.data].B
    pol, qs = _networks(s.data, s.policy, s.policy_activation, s.twins, s.q_activation)
    _install(env, pol, qs)
    _check(name, env, d, pol, qs)


# ---- (b) head and staging widths ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [h.feeder for h in C.HEADS])
def test_head_and_staging_widths_against_the_restatements(name):
    """A = 1 (term stride 1), 2, 5 and 7 (a second Philox quad, partly used), 18 (three head tiles: wavefront 2 owns one); the EVEN
    stage with and without padded columns, two equal panels, four panels.

    Observed on the MI355X: see DESIGN.md section 25 "The edges"."""
    h, f = C.HEAD_CASES[name], C.FEEDERS[name]
    pol, qs = _networks(name)
    env = _env(name, h.B, h.episode_length, h.limits)
    try:
        assert (env.obs_dim, env.action_dim) == (f.D, f.A)
        _install(env, pol, qs)
        d = _collect(env, h.T)
        flags, n = d["terminals"], len(d["terminal_index"])
        rows, ends = C.head_rows(h)
        assert flags.size == rows and n == (flags != 0).sum() >= ends
        if f.D >= C.WIDE_D:                  # the yardstick's counts: only the time limit ends an episode
            assert (flags[flags != 0] == 1).all() and n == ends
        _check(name, env, d, pol, qs)
    finally:
        env.close()


# ---- (c) the head's extremes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stochastic", [True, False], ids=["sampled", "deterministic"])
@pytest.mark.parametrize("name", sorted(C.EXTREMES))
def test_the_heads_extremes_bit_for_bit(name, stochastic):
    """log_std clamped at -20 and at 2, gw_tanh's cap min(|x|, 40) and gw_log(1e-6) at a = +-1 in THIS kernel's head and LDS layout:
    the head is restated operation for operation, so saturation gives no licence to differ, and the twins' values at the saturated
    actions stay within 4 E_ref."""
    c = _dataset("ieee13")
    env, d = c["env"], c["data"]
    pol, qs = _networks("ieee13", bias=C.EXTREMES[name])
    _install(env, pol, qs)
    got = _check(f"extremes-{name}-{'sampled' if stochastic else 'deterministic'}", env, d, pol, qs, stochastic=stochastic, inside=False)
    A = env.action_dim
    for part in ("next", "term"):
        pre, eps = got[f"{part}_pre_head"].reshape(-1, 2 * A), got[f"{part}_noise"].reshape(-1, A)
        seen = C.extremes_reached(pre, eps, got[f"{part}_actions"].reshape(-1, A), got[f"{part}_log_probs"].reshape(-1))
        assert seen["above"] == seen["below"] == len(pre), (part, seen)
    assert np.isfinite(got["td_target"]).all() and np.isfinite(got["q_next_min"]).all()
    sign = 1.0 if name == "high" else -1.0
    assert (got["next_actions"][..., 0] == sign).all()        # the column whose mean lies beyond the cap: exactly +-1.0 in every row


# ---- (d) row and terminal tiles, bit for bit ------------------------------------------------------------------------------------------

def _base():
    """13-bus, B = 65, T = 4, ``episode_length`` 2 under limits nothing reaches: 260 rows, 130 terminal entries"""
    if "base" not in _SHARED:
        b = C.BASE
        pol, qs = _networks(b.feeder)
        env = _env(b.feeder, b.B, b.episode_length, b.limits)
        _SHARED["base"] = c = dict(env=env, pol=pol, qs=qs, ev={})
        _install(env, pol, qs)
        c["data"] = d = _collect(env, b.T)
        flags = d["terminals"]
        assert (flags[flags != 0] == 1).all(), "only the time limit ends an episode"
        assert flags.size == 260 and len(d["terminal_index"]) == (flags != 0).sum() == 130
    return _SHARED["base"]


def _base_evaluation(stochastic):
    c = _base()
    if stochastic not in c["ev"]:
        _install(c["env"], c["pol"], c["qs"])
        c["ev"][stochastic] = TQ._evaluate(c["env"], 3, stochastic=stochastic)
    return c["ev"][stochastic]


def _fresh(name):
    """replay ``name`` on a fresh handle: the base's stored actions of its first T' steps and B' instances uploaded, the observations
    asserted to be the base's bits, evaluated under masks 3, 1 and 0 (download, and which terminal views are there)"""
    if name not in _FRESH:
        r, b, base = C.REPLAY_CASES[name], C.BASE, _base()
        env = _env(b.feeder, r.B, b.episode_length, b.limits)
        try:
            _install(env, base["pol"], base["qs"])
            d = _collect(env, r.T, base["data"]["actions"][:r.T, :r.B])
            for k in ("observations", "next_observations", "rewards", "terminals"):
                assert _same(d[k], np.ascontiguousarray(base["data"][k][:r.T, :r.B])), k
            ev = {}
            for mask in (3, 1, 0):
                got = TQ._evaluate(env, mask, stochastic=r.stochastic)
                view = env.handle.rollout_q_next_arrays()
                ev[mask] = dict(got=got, n_terminal=view["n_terminal"],
                                views={k: None if view[k] is None else view[k].shape for k in TERM_ARRAYS},
                                q_views=[None if v is None else v.shape for v in view["term_q"]])
            _FRESH[name] = dict(data=d, ev=ev)
        finally:
            env.close()
    return _FRESH[name]


def _entries(index):
    return {(int(t), int(b)): e for e, (t, b) in enumerate(index)}


def _assert_rows_of_the_base(got, d, want, base_data, T, B):
    """every output of the replay's rows (t < T, b < B) is the base's row, the terminal entries through (t, b)"""
    for k in ARRAYS:
        assert _same(got[k], np.ascontiguousarray(want[k][:T, :B])), k
    for w in range(2):
        assert _same(got["q_next"][w], np.ascontiguousarray(want["q_next"][w][:T, :B])), w
    where = _entries(base_data["terminal_index"])
    sel = np.array([where[(int(t), int(b))] for t, b in d["terminal_index"]], dtype=np.int64)
    assert _same(d["terminal_obs"], base_data["terminal_obs"][sel])
    for k in TERM_ARRAYS:
        assert _same(got[k], want[k][sel]), k
    for w in range(2):
        assert _same(got["term_q"][w], want["term_q"][w][sel]), w


@pytest.mark.parametrize("stochastic", [True, False], ids=["sampled", "deterministic"])
def test_the_base_of_the_tile_cases_against_the_restatements(stochastic):
    """260 rows in five tiles, a terminal list of 130 entries: two full tiles and two entries"""
    c = _base()
    _install(c["env"], c["pol"], c["qs"])
    got = _check("base", c["env"], c["data"], c["pol"], c["qs"], stochastic=stochastic)
    want = _base_evaluation(stochastic)
    for k in ARRAYS + TERM_ARRAYS:
        assert _same(got[k], want[k]), k


@pytest.mark.parametrize("name", [r.name for r in C.REPLAYS])
def test_row_and_terminal_tiles_bit_for_bit(name):
    """1, 64, 65 and 128 rows; 0, 32, 64 and 65 list entries: a row's outputs depend on that row alone, so every one of them --
    pre-head, action, noise, log-probability, both twins, minimum, td target, the terminal entries through (t, b) -- is the bits the
    260-row evaluation gave it.  An empty list under masks 1 and 3: the count is 0, the terminal arrays are there with length 0,
    and the targets are those of mask 0 (no transition ended an episode)."""
    r, base = C.REPLAY_CASES[name], _base()
    rows, entries = C.replay_rows(r)
    f = _fresh(name)
    d = f["data"]
    assert d["rewards"].size == rows and len(d["terminal_index"]) == entries
    want = _base_evaluation(r.stochastic)
    got = f["ev"][3]["got"]
    if r.stochastic:
        assert np.std(got["next_noise"]) > 0.1
    else:
        assert not got["next_noise"].any()
    _assert_rows_of_the_base(got, d, want, base["data"], r.T, r.B)
    A = base["env"].action_dim
    for mask in (1, 3):
        e = f["ev"][mask]
        assert e["n_terminal"] == entries
        assert e["views"] == dict(term_pre_head=(entries, 2 * A), term_actions=(entries, A), term_noise=(entries, A), term_log_probs=(entries,),
                                  term_q_min=(entries,), term_value=(entries,)) and e["q_views"] == [(entries,), (entries,)]
        assert all(e["got"][k].shape[0] == entries for k in TERM_ARRAYS) and all(q.shape == (entries,) for q in e["got"]["term_q"])
        assert _same(e["got"]["td_target"], TQ._td(d, e["got"], mask, ALPHA))
    zero = f["ev"][0]
    assert all(v is None for v in zero["views"].values()) and zero["q_views"] == [None, None]
    if entries == 0:
        for mask in (1, 3):
            e = f["ev"][mask]["got"]
            assert not d["terminals"].any()
            assert _same(e["td_target"], td_policy_np(d["rewards"], e["next_log_probs"], e["q_next_min"], d["terminals"], [], np.zeros((0, 2)), GAMMA, ALPHA, mask))
            assert _same(e["td_target"], zero["got"]["td_target"])
            for k in ARRAYS:
                assert _same(e[k], zero["got"][k]), k
    else:       # every entry of this rollout ends at the time limit: mask 1 is mask 3, mask 0 differs there
        assert _same(f["ev"][1]["got"]["td_target"], got["td_target"]) and not np.array_equal(zero["got"]["td_target"], got["td_target"])


# ---- (e) buffer reuse -----------------------------------------------------------------------------------------------------------------

def test_a_shorter_and_a_longer_rollout_on_a_handle_that_evaluated_another():
    """The arrays are sized by the rollout's CAPACITY and the second twin lives at ``q + cap``: on one handle the 4-step rollout,
    then 1 step (T < T_cap; 130 stale entries beyond a count of 0, stale targets), then 4 steps again; on a second handle 1 step
    first, then 4 (release and regrow).  Every evaluation is the bits of the fresh handle's, ``q_next[1]`` and the downloaded
    lengths included; after each one the rollout is evaluated once more under another draw, so that the arrays hold other bits
    than the next rollout's when it starts.  One Q step on the policy-action target at n = 33 gives the same bits on both handles and on the base's."""
    base = _base()
    b, acts = C.BASE, base["data"]["actions"]
    want = {"T4": (_base_evaluation(True), base["data"]), "T1": (_fresh("T1-B65")["ev"][3]["got"], _fresh("T1-B65")["data"])}
    mean, std = _normalisation(b.feeder)
    val = P.MLPValue(*L.draw([C.FEEDERS[b.feeder].D, 64, 1], L.SEEDS["value"]), activation="relu", obs_mean=mean, obs_std=std)
    handles = []
    try:
        for seq in C.REUSE:
            env = _env(b.feeder, b.B, b.episode_length, b.limits)
            handles.append(env)
            _install(env, base["pol"], base["qs"])
            for step in seq:
                T = int(step[1:])
                d = _collect(env, T, acts[:T])
                got = TQ._evaluate(env, 3)
                ev, dw = want[step]
                assert len(d["terminal_index"]) == len(dw["terminal_index"]) == (130 if T == 4 else 0)
                for k, v in ev.items():
                    for x, y in zip(v, got[k]) if isinstance(v, list) else [(v, got[k])]:
                        assert x.shape == y.shape, (seq, step, k)
                TQ._assert_equal_evaluations(got, d, ev, dw, b.B)
                # what this rollout leaves behind for the next one is NOT what the next one computes: the rollouts share their
                # first steps, so the bits of the same draw would be the right ones wherever they were read from
                other = TQ._evaluate(env, 3, draw=DRAW + 1)
                for k in ("next_actions", "next_log_probs", "q_next_min", "td_target"):
                    assert not np.array_equal(other[k], got[k]), k
                assert all(not np.array_equal(x, y) for x, y in zip(other["q_next"], got["q_next"]))
        steps = []
        for env in handles + [base["env"]]:
            env.set_value(val)
            P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
            OnPolicyBatches(env, b.B * b.T, policy=base["pol"], adv_norm="none", seed=5, fields=TQ.FIELDS).prepare()
            TQ._evaluate(env, 3)
            learner, out = TQ._q_steps(env, 1, 33, "policy")
            learner.set_q_target("value")
            steps.append(out[0])
        for other in steps[1:]:
            for w in range(2):
                for k in ("params", "grads", "m", "v"):
                    assert _same(steps[0][w][k], other[w][k]), (w, k)
        assert np.abs(steps[0][0]["grads"]).max() > 0.0 and np.abs(steps[0][1]["grads"]).max() > 0.0
    finally:
        for env in handles:
            env.close()
        _install(base["env"], base["pol"], base["qs"])
