"""GPU: constraint costs of a rollout on the device (include/gridstep.h) -- gs_k_costs over a rollout's rows and
its terminal list, gs_costs_eval over crafted rows, the cost critics and their advantages.

Every comparison is np.array_equal (NaN-aware for margins): each quantity is a minimum, a maximum, a count or one rounded subtraction,
so the device's results are the bits of costs_np / rollout_costs_np / gae_np however the kernel maps lanes.  No tolerances.

Environments, policies and critics are built as in tests/test_gpu_onpolicy.py.  The 13-bus feeder's obs_dim is 71 (odd: rows are only
8-byte aligned) and its prefix 51 columns (16 lanes a row, four rows a wavefront pass); the 123-bus feeder's prefix is 491 columns
(64 lanes, two passes of four loads, the second partial)."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.rollout import ConstraintLimits, costs_np, rollout_costs_np, rollout_device

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
WANT = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
KINDS = [("excess", "indicator", "count"), ("indicator", "count", "excess"), ("count", "excess", "indicator")]
V, F, T_ = 0, 1, 2


def _kw(fs, episode_length=5, **extra):
    return dict(solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9, max_iterations=100,
                power_base=fs.base_power_va, episode_length=episode_length, **extra)


def _env(feeder, B, episode_length=5, **extra):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, episode_length, **extra))


_NORM = {}


def _normalisation(feeder):
    """(mean, std) per observation column over a 4-step random rollout of 64 instances; once per feeder"""
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


def _policy(env, feeder, hidden=(100, 37), compute="float32", seed=0):
    ws, bs = _layers([env.obs_dim, *hidden, 2 * env.action_dim], seed)
    mean, std = _normalisation(feeder)
    return P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=mean, obs_std=std, compute=compute)


def _value(env, feeder, hidden=(100, 37), activation="relu", seed=1):
    ws, bs = _layers([env.obs_dim, *hidden, 1], seed)
    mean, std = _normalisation(feeder)
    return P.MLPValue(ws, bs, activation=activation, obs_mean=mean, obs_std=std)


def _random_rollout(env, T, seed=3, policy_seed=7):
    env.reset(seed=seed)
    rollout_device(env, T, seed=policy_seed, reset=False)
    d = env.handle.rollout_download(want=WANT)
    d["state"] = env.get_state()
    return d


def _terminal_index(env):
    return env.handle.rollout_device_arrays()["terminal_index"].to_host()


def _median_limits(d, fs):
    """limits at the medians over the rollout's transitions of the per-row min |V|, max |V|, f and max loading: every channel then has
    transitions on both sides"""
    nxt = d["next_observations"]
    vm, load, f = nxt[..., 0:2 * fs.n:2], np.abs(nxt[..., 2 * fs.n + 1:2 * fs.n + 2 * fs.m:2]), nxt[..., 2 * fs.n + 2 * fs.m]
    return ConstraintLimits(voltage=(float(np.median(vm.min(axis=-1))), float(np.median(vm.max(axis=-1)))),
                            frequency=(float(np.median(f)), float(f.max()) + 1.0), thermal=float(np.median(load.max(axis=-1))))


def _equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _check_rollout_costs(env, fs, d, limits):
    T, B = d["rewards"].shape
    for kinds in KINDS:
        want = rollout_costs_np(d["next_observations"], fs, limits, kinds)
        margins = want[0]
        for c in range(3):                   # a condition on the inputs: both classes in every channel
            assert (margins[c] < 0).any() and (margins[c] >= 0).any(), (c, limits)
        view = P.rollout_costs(env, limits, kinds)
        got = env.handle.rollout_costs_download()
        for k, w in zip(("margins", "counts", "costs", "n_violating"), want):
            assert _equal(getattr(view, k).to_host(), w), (kinds, k, "view")
            assert _equal(got[k], w), (kinds, k, "download")
        assert view.margins.shape == (3, T, B) and 0 < int(want[3].min()) and int(want[3].max()) < T * B
    return want


# ---- 1. the rollout's costs, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [37, 200])
@pytest.mark.parametrize("feeder", ["ieee13", "ieee123"])
def test_rollout_costs_are_rollout_costs_np_bit_for_bit(feeder, B):
    T = 6
    env = _env(feeder, B, episode_length=3)
    fs = env.spec
    assert 2 * fs.n + 2 * fs.m + 1 == {"ieee13": 51, "ieee123": 491}[feeder] and (feeder != "ieee13" or env.obs_dim == 71)
    d = _random_rollout(env, T)
    flags = d["terminals"]
    assert flags[2].all() and flags[5].all() and not flags[[0, 1, 3, 4]].any() and d["n_terminal"] == 2 * B
    # the terminal rows differ from the rows the resets left in their slots: reading the wrong one would show
    obs_seq = np.concatenate([d["observations"], d["final_observation"][None]])
    assert not np.array_equal(obs_seq[3], d["next_observations"][2])
    limits = _median_limits(d, fs)
    _check_rollout_costs(env, fs, d, limits)
    # the defaults are the environment's own limits and 0.8
    dflt = P.rollout_costs(env)
    want = rollout_costs_np(d["next_observations"], fs, ConstraintLimits.of(env), "excess")
    assert _equal(dflt.margins.to_host(), want[0]) and _equal(dflt.costs.to_host(), want[2]) and _equal(dflt.n_violating.to_host(), want[3])
    env.close()


def test_rollout_costs_of_truncated_episodes():
    """every step violates the environment's voltage band, so episodes are truncated once they have more than ten violating steps:
    terminal rows that carry the truncated flag"""
    T = 13
    env = _env("ieee13", 37, episode_length=1000, voltage_limits=(0.99999, 1.00001))
    d = _random_rollout(env, T)
    flags = d["terminals"]
    assert (flags & 2).any() and not (flags & 1).any() and 0 < d["n_terminal"] < T * 37
    _check_rollout_costs(env, env.spec, d, _median_limits(d, env.spec))
    env.close()


# ---- 2. row tiling, ties and NaN through gs_costs_eval ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def eval_envs():
    envs = {f: _env(f, 4) for f in FEEDERS}
    yield envs
    for e in envs.values():
        e.close()


def _crafted(fs, obs_dim, rows, seed):
    n, m = fs.n, fs.m
    W = 2 * n + 2 * m
    rng = np.random.default_rng(seed)
    obs = np.empty((rows, obs_dim))
    obs[:, 0:2 * n:2] = rng.uniform(0.9, 1.1, (rows, n))
    obs[:, 1:2 * n:2] = rng.uniform(-3.0, 3.0, (rows, n))
    obs[:, 2 * n:W:2] = rng.normal(0.0, 1e5, (rows, m))
    obs[:, 2 * n + 1:W:2] = rng.uniform(-1.2, 1.2, (rows, m))
    obs[:, W] = rng.uniform(59.0, 61.0, rows)
    obs[:, W + 1::2], obs[:, W + 2::2] = np.nan, 1e300        # behind the prefix: must not matter
    last = rows - 1
    # ties: the extremes of the last row twice, in the first and the last column of their family
    obs[last, 0] = obs[last, 2 * (n - 1)] = obs[last, 2:2 * (n - 1):2].min()
    obs[last, 2 * n + 1] = -np.abs(obs[last, 2 * n + 3:W - 1:2]).max()
    obs[last, W - 1] = -obs[last, 2 * n + 1]
    obs[last, W] = 60.25
    limits = ConstraintLimits(voltage=(float(obs[last, 0]), 1.1), frequency=(59.5, 60.25), thermal=float(obs[last, W - 1]))
    # NaN in each column family, one row each (rows permitting; never the last row)
    for row, col in enumerate((2, 2 * (n - 1), 1, 2 * n, 2 * n + 3, W - 1, W)):
        if row < last:
            obs[row, col] = np.nan
    return obs, limits


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("feeder", ["ieee13", "ieee123"])
def test_costs_eval_on_crafted_rows(eval_envs, feeder, rows):
    env = eval_envs[feeder]
    fs = env.spec
    obs, limits = _crafted(fs, env.obs_dim, rows, seed=rows)
    for kinds in KINDS:
        got = P.constraint_values(env, obs, limits, kinds)
        margins, counts, costs = costs_np(obs, fs, limits, kinds)
        assert _equal(got["margins"], margins) and _equal(got["counts"], counts) and _equal(got["costs"], costs), kinds
    # the limits sit exactly at the last row's extremes: margin 0, nothing counted, no cost
    assert margins[-1].tolist() == [0.0, 0.0, 0.0] and counts[-1].tolist() == [0, 0, 0] and costs[-1].tolist() == [0.0, 0.0, 0.0]
    if rows > 7:
        nan = np.isnan(margins[:7])
        assert nan[:, V].tolist() == [True, True, False, False, False, False, False]
        assert nan[:, T_].tolist() == [False, False, False, False, True, True, False]
        assert nan[:, F].tolist() == [False] * 6 + [True]
        assert (margins[7:] < 0).any(axis=0).all() and (margins[7:] >= 0).any(axis=0).all()
    # the columns behind the prefix do not matter
    clean = obs.copy()
    clean[:, 2 * fs.n + 2 * fs.m + 1:] = 0.0
    again = P.constraint_values(env, clean, limits, kinds)
    assert _equal(again["margins"], margins) and _equal(again["counts"], counts) and _equal(again["costs"], costs)
    # any output may be left out
    only = env.handle.costs_eval(obs, _lib.cost_config(limits, kinds), want=("counts",))
    assert set(only) == {"counts"} and _equal(only["counts"], counts)


# ---- 3. against the step's own flags -------------------------------------------------------------------------------------------------

def test_constraint_values_agree_with_the_flags_of_env_step():
    B = 37
    env = _env("ieee13", B, episode_length=50, voltage_limits=(0.97, 1.03))
    env.reset(seed=5)
    rng = np.random.default_rng(2)
    vlo, vhi = env.voltage_limits
    seen_v = seen_f = 0
    for step in range(5):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (B, env.action_dim)))
        got = P.constraint_values(env, obs)
        ok = info["power_flow_converged"]
        cv = info["constraint_violations"]
        assert ok.any()
        assert np.array_equal(got["counts"][ok, V] > 0, (cv["voltage_high"] | cv["voltage_low"])[ok])
        assert np.array_equal(got["counts"][ok, F] > 0, (cv["frequency_high"] | cv["frequency_low"])[ok])
        assert np.array_equal(got["margins"][ok, V], np.minimum(info["min_voltage"] - vlo, vhi - info["max_voltage"])[ok])
        seen_v += int((got["counts"][ok, V] > 0).sum())
        seen_f += int((got["counts"][ok, F] > 0).sum())
    print("instances flagged over five steps: voltage", seen_v, "frequency", seen_f)
    assert 0 < seen_v
    env.close()


# ---- 4. cost critics and cost advantages -----------------------------------------------------------------------------------------------

def test_cost_values_and_cost_advantages_are_gae_np_bit_for_bit():
    T, B = 16, 37
    env = _env("ieee13", B, episode_length=7)
    critic, other = _value(env, "ieee13", (100, 37), seed=1), _value(env, "ieee13", (64,), "tanh", seed=2)
    env.set_value(critic)
    env.set_cost_value(0, critic)
    env.set_cost_value("thermal", other)
    d = _random_rollout(env, T)
    flags = d["terminals"]
    assert (flags[6] & 1).all() and not flags[T - 1].any()
    idx = _terminal_index(env)
    limits = _median_limits(d, env.spec)
    reward_values = P.evaluate_rollout(env).values.to_host()
    costs = P.rollout_costs(env, limits, ("excess", "indicator", "count")).costs.to_host()
    gamma, lam, shift, scale = (0.97, 0.5, 0.9), (0.9, 0.5, 0.8), (0.25, 0.0, -0.5), (1.5, 1.0, 0.75)
    for mask in range(4):
        on = P.evaluate_rollout_costs(env, gamma, lam, mask, shift, scale)
        for k in _lib.COST_CRITIC_KEYS:
            assert getattr(on, k)[1] is None and getattr(on, k)[0] is not None and getattr(on, k)[2] is not None
        o = env.handle.rollout_costs_download(_lib.COST_CRITIC_KEYS, channels=(0, 2), n_terminal=d["n_terminal"])
        assert np.array_equal(o["values"][0], reward_values)                # the same network over the same rows: the same bits
        assert not np.array_equal(o["values"][2], reward_values) and o["values"][1] is None
        for c in (0, 2):
            adv, ret = P.gae_np(costs[c], o["values"][c], flags, o["terminal_values"][c], idx, gamma[c], lam[c], mask, shift[c], scale[c])
            assert np.array_equal(o["advantages"][c], adv), (mask, c)
            assert np.array_equal(o["returns"][c], ret), (mask, c)
            assert np.array_equal(getattr(on, "advantages")[c].to_host(), adv) and np.array_equal(on.values[c].to_host(), o["values"][c])
            assert np.array_equal(on.terminal_values[c].to_host(), o["terminal_values"][c]) and np.std(adv) > 0
    view = env.handle.rollout_costs_view()
    assert view.values[1] is None and view.returns[1] is None and view.values[0] and view.advantages[2]
    # scalars reach every channel
    P.evaluate_rollout_costs(env, 0.9, 0.7, ("terminated",), 0.0, 2.0)
    o = env.handle.rollout_costs_download(_lib.COST_CRITIC_KEYS, channels=(2,), n_terminal=d["n_terminal"])
    adv, ret = P.gae_np(costs[2], o["values"][2], flags, o["terminal_values"][2], idx, 0.9, 0.7, 1, 0.0, 2.0)
    assert np.array_equal(o["advantages"][2], adv) and np.array_equal(o["returns"][2], ret)
    env.close()


# ---- 5. nothing else moves ---------------------------------------------------------------------------------------------------------------

def test_costs_and_their_evaluation_leave_everything_else_bit_identical():
    T = 6
    env = _env("ieee13", 37, episode_length=3)
    env.set_policy(_policy(env, "ieee13"), stochastic=True)
    env.set_value(_value(env, "ieee13"))
    for c in range(3):
        env.set_cost_value(c, _value(env, "ieee13", (37,), seed=5 + c))
    env.reset(seed=3)
    rollout_device(env, T, seed=7, reset=False, policy=True)
    P.evaluate_rollout(env, bootstrap=("terminated", "truncated"))

    def snapshot():
        d = env.handle.rollout_download(want=WANT)
        d["state"] = env.get_state()
        d.update(env.handle.rollout_onpolicy_download(n_terminal=d["n_terminal"]))
        return d

    before = snapshot()
    assert before["terminals"].any()
    costs = P.rollout_costs(env, _median_limits(before, env.spec), "count")
    on = P.evaluate_rollout_costs(env, bootstrap=("terminated", "truncated"))
    assert np.isfinite(on.advantages[1].to_host()).all() and costs.costs.to_host().sum() > 0
    after = snapshot()
    assert set(before) == set(after) and len(before) == len(WANT) + 2 + 5
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    env.close()


# ---- 6. state and argument errors ----------------------------------------------------------------------------------------------------------

def _refused(call, code, word):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"error {code}:" in str(e.value) and word in str(e.value), str(e.value)


def test_every_state_and_argument_error():
    S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
    env = _env("ieee13", 5, episode_length=3)
    h = env.handle
    critic = _value(env, "ieee13", (16,))
    good = _lib.cost_config(ConstraintLimits.of(env))
    dflt = h.cost_config_default()
    assert list(dflt.voltage_limits) == list(env.voltage_limits) and list(dflt.frequency_limits) == list(env.frequency_limits)
    assert dflt.line_loading_limit == 0.8 and list(dflt.kind) == [0, 0, 0] and dflt.struct_size == good.struct_size
    env.reset(seed=1)
    _refused(h.rollout_costs, S, "no rollout")
    _refused(h.rollout_evaluate_costs, S, "no rollout")
    _refused(h.rollout_costs_view, S, "no rollout")
    _refused(h.rollout_costs_download, S, "no rollout")
    rollout_device(env, 3, seed=1, reset=False)
    _refused(h.rollout_costs_view, S, "gs_rollout_costs has not run")
    _refused(h.rollout_costs_download, S, "gs_rollout_costs has not run")
    _refused(h.rollout_evaluate_costs, S, "gs_rollout_costs has not run")
    h.rollout_costs()
    _refused(h.rollout_evaluate_costs, S, "before gs_cost_value_mlp_set")
    _refused(lambda: h.rollout_costs_download(("values",), channels=(0,)), S, "channel 0")
    assert h.rollout_costs_view().values[0] is None
    env.set_cost_value(0, critic)
    h.rollout_evaluate_costs()
    _refused(lambda: h.rollout_costs_download(("advantages",), channels=(1,)), S, "channel 1")
    first = h.rollout_costs_download(("margins", "counts", "costs", "n_violating", "advantages"), channels=(0,))
    # argument errors: the previous results and the installed critic stay usable
    _refused(lambda: h.rollout_costs(_lib.cost_config(ConstraintLimits.of(env), struct_size=12)), I, "struct_size")
    _refused(lambda: h.rollout_costs(_lib.cost_config(ConstraintLimits.of(env), (0, 3, 0))), I, "kind[1]")
    _refused(lambda: h.rollout_costs(_lib.cost_config(ConstraintLimits((np.nan, 1.0), (59.5, 60.5), 0.8))), I, "finite")
    _refused(lambda: h.rollout_costs(_lib.cost_config(ConstraintLimits((1.05, 0.95), (59.5, 60.5), 0.8))), I, "voltage_limits: lo > hi")
    _refused(lambda: h.rollout_costs(_lib.cost_config(ConstraintLimits((0.95, 1.05), (60.5, 59.5), 0.8))), I, "frequency_limits: lo > hi")
    _refused(lambda: h.rollout_evaluate_costs(struct_size=8), I, "struct_size")
    _refused(lambda: h.rollout_evaluate_costs(bootstrap_mask=4), I, "bootstrap_mask")
    _refused(lambda: h.rollout_evaluate_costs(gamma=(0.9, np.inf, 0.9)), I, "finite")
    _refused(lambda: h.rollout_evaluate_costs(cost_scale=np.nan), I, "finite")
    for channel in (-1, 3):
        _refused(lambda: env.set_cost_value(channel, critic), I, "channel")
    p, keep = _policy(env, "ieee13", (16,)).to_struct()
    o, keep_o = critic.to_opts()
    _refused(lambda: h.set_cost_value(0, p, o), I, "GS_HEAD_LINEAR")                 # the value network's rules: a Gaussian head
    q, keep_q = critic.to_struct()
    _refused(lambda: h.set_cost_value(0, q, None), I, "GS_COMPUTE_F32")
    _refused(lambda: h.costs_eval(np.zeros((0, env.obs_dim))), I, "rows <= 0")
    lib = _lib.load()
    assert lib.gs_costs_eval(h._h, None, None, 3, None, None, None) == I and b"obs_host is NULL" in lib.gs_last_error(h._h)
    _refused(lambda: h.costs_eval(np.zeros((2, env.obs_dim)), _lib.cost_config(ConstraintLimits.of(env), (0, 0, 7))), I, "kind[2]")
    again = h.rollout_costs_download(("margins", "counts", "costs", "n_violating", "advantages"), channels=(0,))
    for k in ("margins", "counts", "costs", "n_violating"):
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    assert np.array_equal(first["advantages"][0], again["advantages"][0])
    h.rollout_evaluate_costs()                                                      # the critic of channel 0 is still installed
    assert np.array_equal(h.rollout_costs_download(("advantages",), channels=(0,))["advantages"][0], first["advantages"][0])
    # a further rollout: everything is stale, the cost evaluation too
    rollout_device(env, 3, seed=2, reset=False)
    _refused(h.rollout_costs_view, S, "gs_rollout_costs has not run")
    _refused(lambda: h.rollout_costs_download(("margins",)), S, "gs_rollout_costs has not run")
    _refused(h.rollout_evaluate_costs, S, "gs_rollout_costs has not run")
    h.rollout_costs(good)
    _refused(lambda: h.rollout_costs_download(("returns",), channels=(0,)), S, "channel 0")
    assert h.rollout_costs_view().advantages[0] is None and h.rollout_costs_view().T == 3
    h.rollout_evaluate_costs()
    assert h.rollout_costs_view().advantages[0]
    rollout_device(env, 7, seed=2, reset=False)                                     # a longer rollout reallocates: stale, then fine
    _refused(h.rollout_costs_view, S, "gs_rollout_costs has not run")
    h.rollout_costs()
    h.rollout_evaluate_costs()
    assert h.rollout_costs_view().T == 7 and h.rollout_costs_download()["margins"].shape == (3, 7, 5)
    env.set_cost_value(0, None)                                                     # removed: no critic left
    _refused(h.rollout_evaluate_costs, S, "before gs_cost_value_mlp_set")
    env.close()


# ---- 7. collect_constrained_data -----------------------------------------------------------------------------------------------------------

def test_collect_constrained_data_returns_the_documented_keys_in_transition_order():
    T, B = 5, 37
    env = _env("ieee13", B, episode_length=3)
    pol, val = _policy(env, "ieee13"), _value(env, "ieee13")
    critics = {"voltage": _value(env, "ieee13", (37,), seed=8), 2: _value(env, "ieee13", (16,), seed=9)}
    limits = ConstraintLimits.of(env, voltage=(0.98, 1.02), thermal=0.3)
    out = P.collect_constrained_data(env, pol, val, critics, T, seed=4, limits=limits, kinds="count", gamma=0.9, lam=0.8,
                                     bootstrap=("terminated",), cost_gamma=(0.9, 0.9, 0.95), cost_lam=0.7)
    ref = P.collect_onpolicy_data(env, pol, val, T, seed=4, gamma=0.9, lam=0.8, bootstrap=("terminated",))
    assert set(out) == set(ref) | {"constraint_margins", "constraint_costs", "cost_advantages", "cost_returns"}
    for k in ref:
        assert np.array_equal(out[k], ref[k]), k
    margins, counts, costs = costs_np(out["next_observations"], env.spec, limits, "count")
    assert out["constraint_margins"].shape == (T * B, 3) and _equal(out["constraint_margins"], margins) and _equal(out["constraint_costs"], costs)
    assert costs.sum() > 0 and set(out["cost_advantages"]) == set(out["cost_returns"]) == {0, 2}
    # consistent with the views of the same rollout
    view = P.rollout_costs(env, limits, "count")
    on = P.evaluate_rollout_costs(env, (0.9, 0.9, 0.95), 0.7, ("terminated",))
    assert np.array_equal(view.costs.to_host().reshape(3, T * B).T, out["constraint_costs"])
    for c in (0, 2):
        assert out["cost_advantages"][c].shape == (T * B,)
        assert np.array_equal(on.advantages[c].to_host().reshape(T * B), out["cost_advantages"][c])
        assert np.array_equal(on.returns[c].to_host().reshape(T * B), out["cost_returns"][c])
        assert np.array_equal(out["cost_returns"][c], out["cost_advantages"][c] + on.values[c].to_host()[:T].reshape(T * B))
    assert on.values[1] is None
    env.close()
