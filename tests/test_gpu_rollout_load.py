"""GPU: a recorded dataset as the handle's rollout (include/gridstep.h "a recorded dataset as the handle's rollout", DESIGN.md
section 29) -- ``gs_rollout_load`` against the rollout it was downloaded from.

Set-up: the fixtures of tests/test_gpu_q_next.py (``_build``, ``_twin``'s ``_env`` / ``_install``).  X is the handle that collected a
random-action rollout; Y is a second environment of the same spec with the same networks which, before every load, holds ANOTHER rollout
(another seed; asserted to differ from X's, so that no check passes on what was there before).  Shapes: 13-bus T = 37, B = 5,
``episode_length`` 14 (185 rows; both done bits present, asserted); 13-bus T = 4, B = 65, ``episode_length`` 2 (260 rows, 130 of them
terminal; the chunk sizes 1, 64, 65, 259, 260, 261 begin and end mid-step); 123-bus T = 3, B = 70 (684 columns: 64 lanes a row).

No tolerance anywhere: every comparison is by bits.  Arrays indexed by terminal entry are compared after ordering both lists by (t, b):
``gs_rollout`` appends in no particular order, the loader in ascending order."""
import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, gae_np, rollout_device, td_target_np
from tests import test_gpu_q_next as Q

pytestmark = pytest.mark.gpu

# (the 260-row case is this file's: name -> (feeder, B, T, episode_length, hidden widths, activation), as Q.CASES)
Q.CASES.setdefault("ieee13-b65", ("ieee13", 65, 4, 2, [64, 64], "relu"))
CASES = ["ieee13-relu", "ieee13-b65", "ieee123-relu"]
KEYS = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
GAMMA, LAM = Q.GAMMA, 0.95
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
OTHER_SEED = 99


def _same(a, b):
    return Q._same(np.asarray(a), np.asarray(b))


def _download(env):
    return env.handle.rollout_download(want=KEYS)


def _other_rollout(c, y):
    """Y collects a rollout of its own, which is not X's"""
    rollout_device(y, c["T"], seed=OTHER_SEED)
    d = _download(y)
    assert not _same(d["observations"], c["x"]["observations"]) and not _same(d["rewards"], c["x"]["rewards"])


def _load(y, d, **kw):
    return P.load_rollout_data(y, {k: d[k] for k in KEYS if k in d}, **kw)


def _assert_is_x(c, y):
    """test 1's bits: Y's rollout is X's"""
    x, d = c["x"], _download(y)
    for k in KEYS:
        assert _same(d[k], x[k]), k
    assert d["n_terminal"] == x["n_terminal"]
    T, B = c["T"], c["B"]
    dev = y.handle.rollout_device_arrays()
    idx, rows = dev["terminal_index"].to_host(), dev["terminal_obs"].to_host()
    assert len(idx) == x["n_terminal"] == int((x["terminals"] != 0).sum())
    flat = idx[:, 0].astype(np.int64) * B + idx[:, 1]
    assert np.all(np.diff(flat) > 0) and (len(flat) == 0 or (flat[0] >= 0 and flat[-1] < T * B))
    assert np.array_equal(np.flatnonzero(x["terminals"].reshape(-1)), flat)
    assert _same(rows, x["next_observations"][idx[:, 0], idx[:, 1]])
    assert _same(dev["obs_seq"].to_host(), np.concatenate([x["observations"], x["final_observation"][None]]))


_CASES = {}


@pytest.fixture(scope="module")
def case():
    def get(name):
        if name not in _CASES:
            c = dict(Q._build(name))
            c["x"] = _download(c["env"])
            c["y"] = Q._env(c["feeder"], c["B"], c["ep"])
            Q._install(dict(c, env=c["y"]))
            _CASES[name] = c
        return _CASES[name]
    yield get
    for c in _CASES.values():
        c["env"].close()
        c["y"].close()
    _CASES.clear()


# ---- 1. round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_downloaded_rollout_loads_back_bit_for_bit(case, name):
    c = case(name)
    y, x = c["y"], c["x"]
    if name == "ieee13-relu":
        assert (x["terminals"] & 1).any() and (x["terminals"] & 2).any()
    if name == "ieee13-b65":
        assert x["n_terminal"] == 130 and x["terminals"].size == 260
    assert x["n_terminal"] > 0
    _other_rollout(c, y)
    v = _load(y, x)
    assert (v.T, v.B, v.obs_dim, v.action_dim, v.n_terminal) == (c["T"], c["B"], y.obs_dim, y.action_dim, x["n_terminal"])
    _assert_is_x(c, y)
    # the flat time-major dictionary of collect_random_data is the same dataset (no final_observation: next_observations[T - 1])
    _other_rollout(c, y)
    flat = {k: x[k].reshape((-1,) + x[k].shape[2:]) for k in KEYS[:4]}
    flat["terminals"] = x["terminals"].reshape(-1)
    P.load_rollout_data(y, flat)
    d = _download(y)
    assert all(_same(d[k], x[k]) for k in KEYS[:5]) and _same(d["final_observation"], x["next_observations"][-1])


# ---- 2. everything downstream ------------------------------------------------------------------------------------------------------
def _by_tb(idx, B):
    return np.argsort(idx[:, 0].astype(np.int64) * B + idx[:, 1], kind="stable")


def _host(x):
    if x is None:
        return None
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x.to_host() if hasattr(x, "to_host") else x


def _downstream(c, env):
    """what every consumer of "the last rollout" makes of the rollout `env` holds, as host arrays; the terminal arrays ordered by (t, b)"""
    B, pol, h = c["B"], c["pol"], env.handle
    order = _by_tb(h.rollout_device_arrays()["terminal_index"].to_host(), B)
    out = {}
    ev = P.evaluate_rollout(env, gamma=GAMMA, lam=LAM, bootstrap=3)
    out["evaluate"] = dict(values=ev.values.to_host(), terminal_values=ev.terminal_values.to_host()[order], advantages=ev.advantages.to_host(),
                           returns=ev.returns.to_host(), log_probs=_host(ev.log_probs))
    q = P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
    out["q"] = _host(dict(q=q.q, q_min=q.q_min, q_adv=q.q_adv, td_target=q.td_target))
    qn = Q._evaluate(env)
    out["q_next"] = {k: [x[order] for x in v] if isinstance(v, list) and k.startswith("term_") else v[order] if k.startswith("term_") else v for k, v in qn.items()}
    costs = P.rollout_costs(env)
    out["costs"] = _host(dict(margins=costs.margins, counts=costs.counts, costs=costs.costs, n_violating=costs.n_violating))
    ep = P.rollout_episodes(env, start="fresh")
    out["episodes"] = dict(ep.download(), stats={k: np.asarray(v) for k, v in vars(ep.stats).items()}, n=np.asarray(ep.n_episodes))
    ds = P.DeviceGridDataset(env)
    out["dataset"] = dict(stats={k: np.asarray(v) for k, v in ds.raw.items()}, batch=_host(ds.sample_batch(33, seed=4)))
    batches = OnPolicyBatches(env, 64, policy=pol, adv_norm="none", seed=5, fields=Q.FIELDS)
    batches.prepare()
    batch = next(iter(batches.epoch(0)))
    out["minibatch"] = _host({k: v for k, v in batch.items() if v is not None})
    P.refresh_targets(env, batch, ("q_target", "td_value", "q_adv"), gamma=GAMMA, bootstrap=3)
    P.refresh_targets(env, batch, "td_policy", gamma=GAMMA, alpha=Q.ALPHA, bootstrap=3, seed=Q.SEED, draw=Q.DRAW + 1)
    out["refreshed"] = dict(q=h.rollout_q_download(), td_policy=h.rollout_q_next_download(("td_target", "q_next_min", "next_log_probs")))
    # one step of every network in the IQL wiring (examples/device_offline_iql.py)
    nets = ("value", "q1", "q2", "policy")
    learner = P.DeviceLearner(env, nets=nets, **Q.HYPER, policy_loss="awr", temperature=3.0, weight_max=100.0, value_loss="expectile", expectile=0.7,
                              advantage_source="q", value_target="q")
    learner.step(batch)
    out["learner"] = {net: dict(stats={k: np.asarray(v) for k, v in learner.stats(net).items()}, **learner.download(net)) for net in nets}
    return out


def _assert_same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _assert_same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same_tree(x, y, f"{path}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, path
    elif hasattr(a, "__dict__") and not isinstance(a, np.ndarray):          # (a plain host object, such as the episode statistics)
        _assert_same_tree(vars(a), vars(b), path)
    else:
        x, y = np.asarray(a), np.asarray(b)
        if x.dtype.kind in "fiub":
            assert x.dtype == y.dtype and x.shape == y.shape and _same(x.reshape(-1), y.reshape(-1)), path
        else:
            assert a == b, path


@pytest.mark.parametrize("name", CASES)
def test_every_consumer_of_the_last_rollout_gives_the_bits_it_gives_on_the_collecting_handle(case, name):
    c = case(name)
    x_env, y = c["env"], c["y"]
    _other_rollout(c, y)
    Q._install(c)
    Q._install(dict(c, env=y))      # the same networks on both (a learner's step of another test moved them)
    _load(y, c["x"])
    try:
        on_x, on_y = _downstream(c, x_env), _downstream(c, y)
        assert on_x["learner"]["policy"]["stats"]["step"] == 1 and np.isfinite(on_x["learner"]["q1"]["stats"]["value_loss"])
        assert on_x["evaluate"]["terminal_values"].shape == (c["x"]["n_terminal"],) and on_x["episodes"]["n"] == c["x"]["n_terminal"]
        _assert_same_tree(on_x, on_y)
    finally:
        Q._install(c)
        Q._install(dict(c, env=y))


# ---- 3. chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [1, 64, 65, 259, 260, 261, 0])
def test_every_chunking_leaves_the_same_bits(case, chunk_rows):
    c = case("ieee13-b65")
    _other_rollout(c, c["y"])
    _load(c["y"], c["x"], chunk_rows=chunk_rows)
    _assert_is_x(c, c["y"])


@pytest.mark.parametrize("dtype, chunk_rows", [(np.float64, 0), (np.float64, 65), (np.float32, 7)])
def test_a_page_locked_source_is_read_where_it_lies_and_leaves_the_same_bits(case, dtype, chunk_rows):
    """(the copy engine takes a page-locked array's rows straight from it; only the map entries go through the staging)"""
    import ctypes
    c = case("ieee13-b65")
    y, lib, ptrs, src = c["y"], _lib.load(), [], {}
    want = {k: (v.astype(dtype) if v.dtype == np.float64 else v) for k, v in c["x"].items() if k in KEYS}
    try:
        for k, v in want.items():
            p = ctypes.c_void_p()
            assert lib.gs_host_alloc(ctypes.byref(p), max(v.nbytes, 8)) == 0
            ptrs.append(p)
            src[k] = np.frombuffer((ctypes.c_char * v.nbytes).from_address(p.value), dtype=v.dtype, count=v.size).reshape(v.shape)
            src[k][...] = v
        _other_rollout(c, y)
        _load(y, src, chunk_rows=chunk_rows)
        got = _download(y)
        assert all(_same(got[k], want[k].astype(np.float64) if want[k].dtype == np.float32 else want[k]) for k in KEYS)
        if dtype == np.float64:
            _assert_is_x(c, y)
        # ... and a broken row is found there as well
        t, b = (int(v) for v in np.argwhere(c["x"]["terminals"][:-1] == 0)[3])
        src["next_observations"][t, b, 2] = np.nextafter(src["next_observations"][t, b, 2], np.inf)
        Q._refused(lambda: _load(y, src, chunk_rows=chunk_rows), I, f"1 live transition(s) whose next_observations differ from the observation that follows; the first is (t, b) = ({t}, {b})")
    finally:
        del src
        for p in ptrs:
            lib.gs_host_free(p)


# ---- 4. float32 source -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, chunk_rows", [("ieee13-relu", 0), ("ieee13-b65", 7), ("ieee123-relu", 100)])
def test_a_float32_source_is_widened_once_and_exactly(case, name, chunk_rows):
    c = case(name)
    y = c["y"]
    x32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in c["x"].items() if k in KEYS}
    x64 = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in x32.items()}
    assert not _same(x64["observations"], c["x"]["observations"])
    got = []
    for src in (x32, x64):
        _other_rollout(c, y)
        _load(y, src, chunk_rows=chunk_rows)
        dev = y.handle.rollout_device_arrays()
        got.append(dict(_download(y), terminal_obs=dev["terminal_obs"].to_host(), terminal_index=dev["terminal_index"].to_host()))
    _assert_same_tree(got[0], got[1])
    assert all(_same(got[0][k], x64[k]) for k in KEYS)


# ---- 5. more terminals than the simulator's bound ----------------------------------------------------------------------------------
def test_a_dataset_that_ends_an_episode_at_every_transition(case):
    c = case("ieee13-relu")
    y, T, B = c["y"], c["T"], c["B"]
    D, A = y.obs_dim, y.action_dim
    assert T * B > B * (T // min(c["ep"], 11) + 1)              # more entries than gs_rollout's own bound for this handle
    rng = np.random.default_rng(8)
    mean, std = Q._normalisation(c["feeder"])
    d = dict(observations=mean + std * rng.normal(size=(T, B, D)), actions=rng.uniform(-1.0, 1.0, (T, B, A)), rewards=rng.normal(size=(T, B)),
             next_observations=mean + std * rng.normal(size=(T, B, D)), terminals=np.full((T, B), 2, dtype=np.uint8))
    _other_rollout(c, y)
    v = P.load_rollout_data(y, d)
    assert v.n_terminal == T * B
    got = _download(y)
    assert all(_same(got[k], d[k]) for k in d) and _same(got["final_observation"], d["next_observations"][-1]) and got["n_terminal"] == T * B
    idx = y.handle.rollout_device_arrays()["terminal_index"].to_host()
    assert np.array_equal(idx[:, 0].astype(np.int64) * B + idx[:, 1], np.arange(T * B))
    ev = P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=("truncated",))
    values, term_values = ev.values.to_host(), ev.terminal_values.to_host()
    assert term_values.shape == (T * B,) and np.isfinite(term_values).all() and np.ptp(term_values) > 0.0
    adv, ret = gae_np(d["rewards"], values, d["terminals"], term_values, idx, GAMMA, LAM, 2)
    assert _same(ev.advantages.to_host(), adv) and _same(ev.returns.to_host(), ret)
    q = P.evaluate_rollout_q(y, gamma=GAMMA, bootstrap=("truncated",))
    assert _same(q.td_target.to_host(), td_target_np(d["rewards"], values, d["terminals"], term_values, idx, GAMMA, 2))
    # ... and under no bootstrap every target is the reward alone
    P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=())
    assert _same(P.evaluate_rollout_q(y, gamma=GAMMA, bootstrap=()).td_target.to_host(), td_target_np(d["rewards"], values, d["terminals"], term_values, idx, GAMMA, 0))


# ---- 6. capacity, and the simulator afterwards -------------------------------------------------------------------------------------
def _kw(fs):
    return dict(solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9, max_iterations=100,
                power_base=fs.base_power_va, episode_length=14, voltage_limits=(0.98, 1.02))


@pytest.mark.parametrize("per_instance_loads", [False, True])
def test_the_simulator_s_next_rollout_after_loads_of_other_lengths_and_constants(per_instance_loads):
    fs, B = P.ieee13_like("epsilon"), 5
    extra = dict(load_powers=P.randomized_load_powers(fs, B, 0.6, 1.4, seed=3)) if per_instance_loads else {}
    make = lambda: P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs), **extra)
    z, source, twin = make(), make(), make()
    try:
        rollout_device(source, 8, seed=5)
        d8 = source.handle.rollout_download(want=KEYS)
        rollout_device(z, 4, seed=6)                              # T_cap = 4
        P.load_rollout_data(z, d8)                                # longer than the buffers: they are made again
        assert all(_same(z.handle.rollout_download(want=KEYS)[k], d8[k]) for k in KEYS)
        d1 = {k: d8[k][:1] for k in KEYS[:5]}                     # shorter: T = 1 in buffers of 8
        P.load_rollout_data(z, d1)
        got = z.handle.rollout_download(want=KEYS)
        assert got["observations"].shape[0] == 1 and all(_same(got[k], d1[k]) for k in d1) and _same(got["final_observation"], d1["next_observations"][0])
        # the columns no step ever writes: the same in every slot of an instance
        seq = np.concatenate([d8["observations"], d8["final_observation"][None]])
        const = (seq == seq[0]).all(axis=(0, 1))
        assert const.any() and not const.all()
        shifted = {k: d8[k].copy() for k in KEYS}
        for k in ("observations", "next_observations", "final_observation"):
            shifted[k][..., const] += 1.0
        P.load_rollout_data(z, shifted)
        assert _same(z.handle.rollout_download(want=("observations",))["observations"], shifted["observations"])
        rollout_device(z, 4, seed=12)
        rollout_device(twin, 4, seed=12)                          # a handle that never loaded
        a, b = z.handle.rollout_download(want=KEYS), twin.handle.rollout_download(want=KEYS)
        assert a["n_terminal"] == b["n_terminal"] and all(_same(a[k], b[k]) for k in KEYS)
        # ... and the one after that, without a reset in between
        rollout_device(z, 3, seed=13, reset=False)
        rollout_device(twin, 3, seed=13, reset=False)
        a, b = z.handle.rollout_download(want=KEYS), twin.handle.rollout_download(want=KEYS)
        assert all(_same(a[k], b[k]) for k in KEYS)
    finally:
        for e in (z, source, twin):
            e.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def _flip(x, t, b, col):
    x[t, b, col] = np.nextafter(x[t, b, col], np.inf)


def test_a_broken_live_transition_is_refused_with_its_place_and_leaves_no_rollout(case):
    c = case("ieee13-relu")
    y, x, T, B = c["y"], c["x"], c["T"], c["B"]
    live = np.argwhere(x["terminals"] == 0)
    inner = live[live[:, 0] < T - 1]
    last = live[live[:, 0] == T - 1]
    assert len(inner) > 3 and len(last) > 0

    def refused(d, count, t, b, **kw):
        _other_rollout(c, y)
        Q._refused(lambda: _load(y, d, **kw), I, f"{count} live transition(s)")
        Q._refused(lambda: _load(y, d, **kw), I, f"(t, b) = ({t}, {b})")
        Q._refused(lambda: y.handle.rollout_download(), S, "no rollout")
        Q._refused(lambda: y.handle.rollout_device_view(), S, "no rollout")
        Q._refused(lambda: y.handle.dataset_build(), S, "")

    t, b = (int(v) for v in inner[len(inner) // 2])
    d = {k: v.copy() for k, v in x.items() if k in KEYS}
    _flip(d["next_observations"], t, b, 7)
    refused(d, 1, t, b)
    refused(d, 1, t, b, chunk_rows=3)
    # the last step against a given final observation
    tl, bl = (int(v) for v in last[-1])
    d = {k: v.copy() for k, v in x.items() if k in KEYS}
    _flip(d["next_observations"], tl, bl, y.obs_dim - 1)
    refused(d, 1, tl, bl)
    # ... which without one IS the final observation: accepted
    _other_rollout(c, y)
    _load(y, {k: v for k, v in d.items() if k != "final_observation"})
    assert _same(_download(y)["final_observation"], d["next_observations"][-1])
    # two broken rows: the lower index is named, in whichever chunk it lies
    (t0, b0), (t1, b1) = (tuple(int(v) for v in r) for r in (inner[1], inner[-2]))
    assert t0 * B + b0 < t1 * B + b1
    d = {k: v.copy() for k, v in x.items() if k in KEYS}
    _flip(d["next_observations"], t1, b1, 0)
    _flip(d["next_observations"], t0, b0, 0)
    refused(d, 2, t0, b0)
    refused(d, 2, t0, b0, chunk_rows=11)
    # a NaN equals the same NaN; a done row may hold anything
    d = {k: v.copy() for k, v in x.items() if k in KEYS}
    d["next_observations"][t, b, 3] = d["observations"][t + 1, b, 3] = np.nan
    td, bd = (int(v) for v in np.argwhere(x["terminals"] != 0)[0])
    d["next_observations"][td, bd] = -7.0
    _other_rollout(c, y)
    _load(y, d)
    got = _download(y)
    assert _same(got["next_observations"], d["next_observations"]) and _same(got["observations"], d["observations"])


# ---- 8. staleness and log-probabilities --------------------------------------------------------------------------------------------
def test_a_load_is_a_new_rollout_and_records_log_probabilities_only_when_given(case):
    c = case("ieee13-relu")
    y, x, h = c["y"], c["x"], c["y"].handle
    Q._install(dict(c, env=y))
    _other_rollout(c, y)
    P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=3)
    P.evaluate_rollout_q(y, gamma=GAMMA, bootstrap=3)
    Q._evaluate(y)
    P.rollout_costs(y)
    P.rollout_episodes(y, start="fresh")
    ds = P.DeviceGridDataset(y)
    for view in (h.rollout_q_arrays, h.rollout_q_next_arrays, h.rollout_onpolicy_arrays, h.rollout_costs_arrays, h.rollout_episodes_arrays):
        view()
    _load(y, x)
    for view in (h.rollout_q_arrays, h.rollout_q_next_arrays, h.rollout_onpolicy_arrays, h.rollout_costs_arrays, h.rollout_episodes_arrays,
                 lambda: ds.sample_batch(8, seed=1), lambda: h.onpolicy_batch(5, 0, 0, 8)):
        Q._refused(view, S, "")
    P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=3)
    assert P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=3).log_probs is None
    P.evaluate_rollout_q(y, gamma=GAMMA, bootstrap=3)
    h.rollout_q_arrays()
    ds.rebuild(keep_stats=True)
    ds.sample_batch(8, seed=1)
    batches = OnPolicyBatches(y, 64, policy=c["pol"], adv_norm="none", seed=5, fields=Q.FIELDS)
    batches.prepare()
    batch = next(iter(batches.epoch(0)))
    learner = P.DeviceLearner(y, nets=("policy",), **Q.HYPER)
    Q._refused(lambda: learner.step(batch), S, "recorded no log-probabilities")
    learner.set_loss("policy", "awr", temperature=1.0, weight_max=20.0)
    learner.step(batch)
    assert learner.stats("policy")["step"] == 1
    Q._install(dict(c, env=y))
    # a stochastic rollout's log-probabilities travel with it
    e = Q._env(c["feeder"], c["B"], c["ep"])
    try:
        Q._install(dict(c, env=e))
        rollout_device(e, 6, seed=3, policy=True)
        d = P.download_rollout(e)
        assert "log_probs" in d and d["log_probs"].shape == (6, c["B"]) and np.isfinite(d["log_probs"]).all()
        _other_rollout(c, y)
        P.load_rollout_data(y, d)
        assert _same(P.evaluate_rollout(y, gamma=GAMMA, lam=LAM, bootstrap=3).log_probs.to_host(), d["log_probs"])
        assert _same(P.download_rollout(y)["log_probs"], d["log_probs"])
        # ... and a load without them says so again
        P.load_rollout_data(y, {k: v for k, v in d.items() if k != "log_probs"})
        assert "log_probs" not in P.download_rollout(y)
    finally:
        e.close()


# ---- 9. the environment is not touched ---------------------------------------------------------------------------------------------
def test_the_environment_steps_on_as_if_nothing_had_been_loaded(case):
    c = case("ieee13-relu")
    x = c["x"]
    y, twin = Q._env(c["feeder"], c["B"], c["ep"]), Q._env(c["feeder"], c["B"], c["ep"])
    try:
        _load(y, x)                                   # a handle that was never reset may load
        assert all(_same(_download(y)[k], x[k]) for k in KEYS)
        actions = np.random.default_rng(4).uniform(-1.0, 1.0, (2, c["B"], y.action_dim))
        for env in (y, twin):
            env.reset(seed=21)
        a0, b0 = y.step(actions[0]), twin.step(actions[0])
        _load(y, x, chunk_rows=17)                    # mid-episode
        a1, b1 = y.step(actions[1]), twin.step(actions[1])
        for a, b in ((a0, b0), (a1, b1)):
            assert all(_same(p, q) for p, q in zip(a[:4], b[:4]))
        assert all(_same(_download(y)[k], x[k]) for k in KEYS)      # and stepping left the loaded rollout alone
    finally:
        y.close()
        twin.close()
