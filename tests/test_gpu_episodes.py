"""Episode accounting on the device: ``gs_rollout_episodes`` against ``episodes_np`` bit for bit over chains of
rollouts, both kinds of episode end, episodic costs, the statistics against ``math.fsum`` within the bound of the reduction order,
the order of the list, the state rules, non-interference, and ``evaluate_policy``."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.rollout import ConstraintLimits, episodes_np, evaluate_policy, evaluate_rollout, rollout_costs, rollout_episodes

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
KINDS = [("excess", "indicator", "count"), ("indicator", "count", "excess"), ("count", "excess", "indicator")]
LIST = ("episode_index", "episode_return", "episode_length", "episode_ordinal", "episode_flags")
LIST_COSTS = ("episode_cost", "episode_violating", "episode_any_violating")
CARRY = ("ep_return", "ep_length", "ep_ordinal", "ep_partial")
CARRY_COSTS = ("ep_cost", "ep_violating", "ep_any_violating")
U = 2.0 ** -53


def _env(feeder, B, episode_length=5, **extra):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=episode_length, **extra)


def _layers(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


def _actor(env, hidden=(32,), seed=0):
    """a fixed small actor; observations normalised by one reset's own columns"""
    obs, _ = env.reset(seed=1)
    mean, std = obs.mean(axis=0), obs.std(axis=0)
    ws, bs = _layers([env.obs_dim, *hidden, 2 * env.action_dim], seed)
    return P.MLPPolicy(ws, bs, activation="tanh", head="gaussian_tanh", obs_mean=mean, obs_std=np.where(std <= 1e-9, 1.0, std + 1e-6), compute="float32")


def _value(env, hidden=(32,), seed=1):
    ws, bs = _layers([env.obs_dim, *hidden, 1], seed)
    return P.MLPValue(ws, bs, activation="tanh")


def _equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _stagger(env, seed=3):
    """instances at three different points of their episodes: two one-step rollouts with a masked reset after each"""
    B = env.num_envs
    env.reset(seed=seed)
    for k in (0, 1):
        env.handle.rollout(1, "random", seed=90 + k)
        env.reset(seed=seed + 100 * (k + 1), mask=(np.arange(B) % 3 == k))


def _account_and_compare(env, start, carry, costs=False, success_return=-1000.0, tag=""):
    """accounts the last rollout on the device and with ``episodes_np`` over the downloaded arrays; every list array, every carry and
    the view's arrays bit for bit; returns (device download, np records, np stats, np carry, EpisodeRecords)"""
    h = env.handle
    d = h.rollout_download(("rewards", "terminals"))
    c = h.rollout_costs_download(("margins", "costs")) if costs else {}
    rec, stats, new_carry = episodes_np(d["rewards"], d["terminals"], c.get("costs"), c.get("margins"), carry=carry, start=start, success_return=success_return)
    view = rollout_episodes(env, start, costs, success_return)
    got = view.download()
    n = d["n_terminal"]
    assert got["n_episodes"] == n == view.n_episodes == len(rec["episode_return"]), tag
    for k in LIST + (LIST_COSTS if costs else ()):
        assert _equal(got[k], rec[k]), (tag, k, "download")
        dev = getattr(view, k)
        dev = np.stack([x.to_host() for x in dev]) if isinstance(dev, list) else dev.to_host()
        assert _equal(dev, rec[k]), (tag, k, "view")
    for k in CARRY + (CARRY_COSTS if costs else ()):
        assert _equal(got[k], new_carry[k]), (tag, k, "download")
        assert _equal(getattr(view, k).to_host(), new_carry[k]), (tag, k, "view")
    if not costs:
        assert all(getattr(view, k) is None for k in LIST_COSTS + CARRY_COSTS), tag
    # sorted by (b, t_end), and the rollout's own terminal list as a set
    idx = rec["episode_index"]
    assert np.array_equal(np.lexsort((idx[:, 0], idx[:, 1])), np.arange(n)), tag
    term = h.rollout_device_arrays()["terminal_index"].to_host()
    assert sorted(map(tuple, term.tolist())) == sorted(map(tuple, idx.tolist())), tag
    assert view.stats.count == stats.count and view.stats.count_partial == stats.count_partial, tag
    return got, rec, stats, new_carry, view


# ---- 1. the list and the carries, bit for bit, over chains of rollouts -------------------------------------------------------------------

@pytest.mark.parametrize("feeder,B,episode_length,T,rollouts,stagger", [
    ("ieee13", 1, 5, 7, 3, False), ("ieee13", 37, 5, 7, 3, False), ("ieee13", 200, 5, 7, 3, True),     # episodes straddle every boundary
    ("ieee13", 37, 3, 1, 3, False),                                                                   # a one-step rollout
    ("ieee13", 37, 1000, 13, 3, False),                                                               # no episode ends
    ("ieee13", 1025, 3, 4, 1, True), ("ieee13", 2049, 3, 4, 1, True),                                 # the offset pass: chunk carry, partial last chunk
    ("ieee123", 37, 5, 7, 3, False)])
def test_episode_list_and_carries_are_episodes_np_bit_for_bit(feeder, B, episode_length, T, rollouts, stagger):
    env = _env(feeder, B, episode_length=episode_length)
    if stagger:
        _stagger(env)
    else:
        env.reset(seed=3)
    carry, total, per_instance = None, 0, np.zeros(B, dtype=np.int64)
    for r in range(rollouts):
        env.handle.rollout(T, "random", seed=7 + r)
        start = ("unknown" if stagger else "fresh") if r == 0 else "continue"
        got, rec, stats, carry, view = _account_and_compare(env, start, carry, tag=(feeder, B, r))
        total += got["n_episodes"]
        np.add.at(per_instance, rec["episode_index"][:, 1], 1)
        if stagger and r == 0:          # exactly each instance's first record is partial
            assert np.array_equal((rec["episode_flags"] & 4) != 0, rec["episode_ordinal"] == 0) and stats.count_partial > 0
        elif not stagger:
            assert not (rec["episode_flags"] & 4).any()
    if episode_length == 1000:
        assert total == 0 and carry["ep_length"].tolist() == [T * rollouts] * B and math.isnan(view.stats.return_mean) and view.stats.count == 0
    else:
        assert total > 0 and np.array_equal(carry["ep_ordinal"], per_instance)
    if stagger and rollouts == 1:       # instances finished different numbers of episodes: the offsets are no multiple of b
        assert len(set(per_instance.tolist())) > 1
    if episode_length == 5 and not stagger:      # T = 7 against 5: an episode straddles every boundary between the rollouts
        assert carry["ep_length"].tolist() == [(T * rollouts) % 5] * B
    env.close()


# ---- 2. both kinds of episode end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["terminated", "truncated"])
def test_record_flags_are_the_done_flags_bits(kind):
    if kind == "terminated":
        env, T, bit = _env("ieee13", 37, episode_length=7), 16, 1
    else:       # every step violates the voltage band: truncated once an episode has more than ten violating steps
        env, T, bit = _env("ieee13", 37, episode_length=1000, voltage_limits=(0.99999, 1.00001)), 13, 2
    env.reset(seed=3)
    env.handle.rollout(T, "random", seed=7)
    got, rec, stats, carry, view = _account_and_compare(env, "fresh", None, tag=kind)
    d = env.handle.rollout_download(("terminals",))
    flags = rec["episode_flags"]
    assert len(flags) > 0 and (flags & bit).all() and not (flags & (3 ^ bit)).any() and not (flags & 4).any()
    assert np.array_equal(flags, d["terminals"][rec["episode_index"][:, 0], rec["episode_index"][:, 1]].astype(np.int32))
    env.close()


# ---- 3. episodic costs ----------------------------------------------------------------------------------------------------------------

def _some_violations(next_obs, fs):
    """limits that a fifth of the transitions violate in the voltage channel and a twentieth in the thermal one (the frequency band is
    the default one): episodes with a violating step and episodes without"""
    vm, load = next_obs[..., 0:2 * fs.n:2], np.abs(next_obs[..., 2 * fs.n + 1:2 * fs.n + 2 * fs.m:2])
    return ConstraintLimits(voltage=(float(np.quantile(vm.min(axis=-1), 0.2)), 2.0), frequency=(59.5, 60.5),
                            thermal=float(np.quantile(load.max(axis=-1), 0.95)))


def test_episodic_costs_are_episodes_np_bit_for_bit_for_every_cost_kind():
    B, T = 37, 7
    env = _env("ieee13", B, episode_length=3)
    env.reset(seed=3)
    carry, limits, any_viol, any_clean, successes = None, None, False, False, 0
    for r, kinds in enumerate(KINDS):
        env.handle.rollout(T, "random", seed=7 + r)
        if limits is None:
            limits = _some_violations(env.handle.rollout_download(("next_observations",))["next_observations"], env.spec)
        rollout_costs(env, limits, kinds)
        floor = -np.inf if r == 0 else float(np.median(env.handle.rollout_download(("rewards",))["rewards"]) * 3)
        got, rec, stats, carry, view = _account_and_compare(env, "fresh" if r == 0 else "continue", carry, costs=True, success_return=floor, tag=kinds)
        assert view.stats.n_success == stats.n_success == int(np.sum((rec["episode_any_violating"] == 0) & (rec["episode_return"] > floor)))
        assert np.array_equal(view.stats.violating, stats.violating) and (stats.violating == rec["episode_violating"].sum(axis=1)).all()
        any_viol |= bool((rec["episode_any_violating"] > 0).any()); any_clean |= bool((rec["episode_any_violating"] == 0).any())
        successes += stats.n_success
        assert (rec["episode_cost"] > 0).any()
    assert any_viol and any_clean and successes > 0
    env.close()


# ---- 4. the statistics -----------------------------------------------------------------------------------------------------------------

def _stat_bounds(n_list, xs):
    """d = ceil(n_list / 1024) - 1 + 10 additions on the longest path of the sum"""
    d = -(-n_list // 1024) - 1 + 10
    n = len(xs)
    mean = math.fsum(xs) / n
    std = math.sqrt(math.fsum((x - mean) ** 2 for x in xs) / n)
    mean_bound = (d + 2) * U * math.fsum(abs(x) for x in xs) / n
    return mean, std, mean_bound, (d / 2 + 3) * U * std + mean_bound


def _prepared(B, T, with_costs):
    env = _env("ieee13", B, episode_length=3)
    _stagger(env)
    env.handle.rollout(T, "random", seed=7)
    if with_costs:
        rollout_costs(env, _some_violations(env.handle.rollout_download(("next_observations",))["next_observations"], env.spec), "excess")
    return env


@pytest.mark.parametrize("with_costs", [False, True])
def test_statistics_match_fsum_within_the_bound_of_the_reduction_order(with_costs):
    B, T = 700, 10      # ~2300 records: the statistics workgroup's threads hold two or three each
    env, twin = _prepared(B, T, with_costs), _prepared(B, T, with_costs)
    got, rec, stats, carry, view = _account_and_compare(env, "unknown", None, costs=with_costs, success_return=-1e300)
    s = view.stats
    full = (rec["episode_flags"] & 4) == 0
    xs, lens = rec["episode_return"][full].tolist(), rec["episode_length"][full]
    n_list = len(full)
    assert n_list > 2048 and s.count == len(xs) > 1000 and s.count_partial == n_list - len(xs) > 0
    assert s.return_min == min(xs) and s.return_max == max(xs)
    assert s.length_min == lens.min() and s.length_max == lens.max() and s.length_mean == float(lens.sum()) / len(xs)
    mean, std, mean_bound, std_bound = _stat_bounds(n_list, xs)
    ratios = [abs(s.return_mean - mean) / mean_bound, abs(s.return_std - std) / std_bound]
    if with_costs:
        clean = rec["episode_any_violating"][full] == 0
        assert s.n_success == int(clean.sum()) and 0 < s.n_success < len(xs)
        assert s.violating.tolist() == rec["episode_violating"][:, full].sum(axis=1).tolist() and s.violating[0] > 0
        for c in range(3):
            cs = rec["episode_cost"][c][full].tolist()
            cmean, _, cbound, _ = _stat_bounds(n_list, cs)
            ratios.append(abs(s.cost_mean[c] - cmean) / cbound if cbound else float(s.cost_mean[c] != cmean))
    else:
        assert s.n_success == len(xs) and np.isnan(s.cost_mean).all() and s.violating.tolist() == [0, 0, 0]
    print(f"episode statistics, costs {with_costs}: n {len(xs)}, observed error / bound {['%.3g' % x for x in ratios]}, largest {max(ratios):.3g}")
    assert max(ratios) <= 1.0, ratios
    # an identically prepared handle: the same bits
    again = rollout_episodes(twin, "unknown", with_costs, -1e300)
    a = env.handle.rollout_episodes_download(("stats",))["stats"]
    b = twin.handle.rollout_episodes_download(("stats",))["stats"]
    assert ctypes.string_at(ctypes.addressof(a), ctypes.sizeof(a)) == ctypes.string_at(ctypes.addressof(b), ctypes.sizeof(b))
    assert again.stats.count == s.count
    # determinism of the order: the same seeds, the same list
    assert _equal(again.download(("episode_index",))["episode_index"], rec["episode_index"])
    env.close(); twin.close()


# ---- 5. the state rules ----------------------------------------------------------------------------------------------------------------

def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_state_rules_and_refusals_leave_the_carries_alone():
    S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
    B, T = 37, 4
    env = _env("ieee13", B, episode_length=3)
    h = env.handle
    cfg = _lib.episode_config
    env.reset(seed=3)
    _refused(lambda: h.rollout_episodes(cfg("fresh")), S, "no rollout has been collected")
    h.rollout(T, "random", seed=7)
    _refused(lambda: h.rollout_episodes_view(), S, "gs_rollout_episodes has not run on the last rollout")
    _refused(lambda: h.rollout_episodes_download(("ep_return",)), S, "gs_rollout_episodes has not run on the last rollout")
    _refused(lambda: h.rollout_episodes(cfg("continue")), S, "without an episode track")
    _refused(lambda: h.rollout_episodes(None), S, "without an episode track")          # NULL: continue
    _refused(lambda: h.rollout_episodes(cfg("fresh", struct_size=8)), I, "struct_size")
    _refused(lambda: h.rollout_episodes(cfg(3)), I, "start")
    _refused(lambda: h.rollout_episodes(cfg("fresh", success_return=np.nan)), I, "success_return")
    _refused(lambda: h.rollout_episodes(cfg("fresh", success_return=np.inf)), I, "success_return")
    _refused(lambda: h.rollout_episodes(cfg("fresh", costs=True)), S, "gs_rollout_costs has not run on the last rollout")
    got, rec, stats, carry, view = _account_and_compare(env, "fresh", None, success_return=-np.inf, tag="first")      # (-inf is accepted)
    assert stats.n_success == stats.count > 0
    _refused(lambda: h.rollout_episodes(cfg("continue")), S, "already been accounted")
    _refused(lambda: h.rollout_episodes(cfg("fresh")), S, "already been accounted")
    # a further rollout: refusals first, then the carries continue as if nothing had been asked
    h.rollout(T, "random", seed=8)
    _refused(lambda: h.rollout_episodes_view(), S, "has not run on the last rollout")
    _refused(lambda: h.rollout_episodes(cfg("continue", costs=True)), S, "track started with 0")
    h.rollout_costs()
    _refused(lambda: h.rollout_episodes(cfg("continue", costs=True)), S, "track started with 0")
    _refused(lambda: h.rollout_episodes(cfg("continue", struct_size=0)), I, "struct_size")
    _refused(lambda: h.rollout_episodes(cfg("continue", success_return=np.nan)), I, "success_return")
    got, rec, stats, carry, view = _account_and_compare(env, "continue", carry, tag="second")
    assert (rec["episode_length"] == 3).all() and len(rec["episode_length"]) > 0        # carried over the boundary: whole episodes
    # a rollout that was not accounted breaks the chain
    h.rollout(T, "random", seed=9)
    h.rollout(T, "random", seed=10)
    _refused(lambda: h.rollout_episodes(cfg("continue")), S, "was not accounted")
    got, rec, stats, carry, view = _account_and_compare(env, "unknown", None, tag="restart")
    assert stats.count_partial == B
    # the environment moved outside gs_rollout
    for move in ("step", "reset", "set_state"):
        if move == "step":
            env.step(np.zeros((B, env.action_dim)))
        elif move == "reset":
            env.reset(seed=5)
        else:
            env.set_state(env.get_state())
        h.rollout(T, "random", seed=11)
        _refused(lambda: h.rollout_episodes(cfg("continue")), S, "moved outside gs_rollout")
        got, rec, stats, carry, view = _account_and_compare(env, "fresh" if move == "reset" else "unknown", None, tag=move)
    h.rollout(T, "random", seed=12)
    h.episodes_clear()
    _refused(lambda: h.rollout_episodes(cfg("continue")), S, "without an episode track")
    _refused(lambda: h.rollout_episodes_view(), S, "has not run on the last rollout")
    _account_and_compare(env, "unknown", None, tag="after clear")
    env.close()


# ---- 6. non-interference ---------------------------------------------------------------------------------------------------------------

def test_accounting_leaves_the_environment_and_the_rollout_as_they_were():
    B, T = 37, 7
    want = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
    envs = [_env("ieee13", B, episode_length=5) for _ in range(2)]
    actor = _actor(envs[0])
    for e in envs:
        e.set_policy(actor, stochastic=True)
        e.set_value(_value(e))
        e.reset(seed=3)
    for r in range(2):
        for e in envs:
            e.handle.rollout(T, "mlp", seed=7 + r)
        busy, plain = envs
        rollout_costs(busy)
        rollout_episodes(busy, "fresh" if r == 0 else "continue", costs=True)
        on = evaluate_rollout(busy)
        a, b = busy.handle.rollout_download(want), plain.handle.rollout_download(want)
        for k in want:
            assert _equal(a[k], b[k]), (r, k)
        assert a["n_terminal"] == b["n_terminal"]
        assert _equal(busy.get_state(), plain.get_state()), r
        assert _equal(busy.handle.rollout_onpolicy_download(("log_probs",))["log_probs"], plain.handle.rollout_onpolicy_download(("log_probs",))["log_probs"])
        assert on.advantages.shape == (T, B)
        # get_state() is no move of the environment: the chain goes on
    for e in envs:
        e.close()


# ---- 7. evaluate_policy ----------------------------------------------------------------------------------------------------------------

def test_evaluate_policy_counts_each_instances_first_episodes():
    B, K, T, seed = 37, 2, 4, 21
    env = _env("ieee13", B, episode_length=5)
    actor = _actor(env)
    out = evaluate_policy(env, actor, episodes_per_instance=K, seed=seed, limits=ConstraintLimits.of(env), rollout_steps=T)
    assert out["episode_returns"].shape == (B * K,) and out["episodes"] == B * K and out["episode_lengths"].tolist() == [5] * (B * K)
    assert out["steps"] == 12 and out["mean_cost"].shape == (3,) and 0.0 <= out["success_rate"] <= 1.0 and out["safety_violations"] >= 0
    assert out["mean_return"] == float(np.mean(out["episode_returns"])) and out["std_return"] == float(np.std(out["episode_returns"]))
    # the same seeds by hand: downloaded rollouts, the host's restatement
    twin = _env("ieee13", B, episode_length=5)
    twin.reset(seed=seed)
    twin.set_policy(actor, stochastic=False)
    want, carry = [], None
    for r in range(3):
        twin.handle.rollout(T, "mlp", seed=seed + r)
        d = twin.handle.rollout_download(("rewards", "terminals"))
        rec, _, carry = episodes_np(d["rewards"], d["terminals"], carry=carry, start="fresh" if r == 0 else "continue")
        want.append(rec["episode_return"][rec["episode_ordinal"] < K])
    assert _equal(out["episode_returns"], np.concatenate(want))
    plain = evaluate_policy(twin, actor, episodes_per_instance=K, seed=seed, rollout_steps=T)
    assert _equal(plain["episode_returns"], out["episode_returns"]) and plain["safety_violations"] is None and plain["mean_cost"] is None
    with pytest.raises(PowerFlowError, match="max_steps"):
        evaluate_policy(env, actor, episodes_per_instance=K, seed=seed, rollout_steps=T, max_steps=8)
    env.close(); twin.close()
