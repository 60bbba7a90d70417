"""GPU: a sliding window over consecutive rollouts (include/gridstep.h "a sliding window over consecutive rollouts", DESIGN.md section
30) -- ``gs_rollout_continue`` against ONE long ``gs_rollout`` from the same reset seeds.

13-bus feeder, B = 70 (one full group of 64 instances and a ragged one), ``episode_length`` 4 so that episodes end in the dropped, the
kept and the new part; T1 = 7 steps, then continues of T2 = 5.  Three modes: the second-generation step kernels with their fused
bookkeeping ("fused"), ``GS_NO_FLOW2=1`` (the small kernel after every step: "post"), and a stochastic float32 MLP policy with recorded
log-probabilities ("mlp").  Per mode one environment collects the long rollout of T1 + 3 T2 steps once -- the reference every test
slices -- and, having the capacity for it, shifts IN PLACE afterwards; the growth test uses an environment of its own.

No tolerance anywhere: every comparison is by bits.  Terminal lists are compared as sorted (t, b, row) sets: ``gs_rollout`` appends in
no particular order."""
import ctypes

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, continue_rollout, episodes_np, rollout_device, rollout_episodes
from tests import test_gpu_q_next as Q

pytestmark = pytest.mark.gpu

B, EP, T1, T2, LONG = 70, 4, 7, 5, 7 + 3 * 5
RESET_SEED, SEED = 3, 7
MODES = ["fused", "post", "mlp"]
KEYS = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
GAMMA, LAM = Q.GAMMA, 0.95
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID


def _same(a, b):
    return Q._same(np.asarray(a), np.asarray(b))


def _env(num_envs=B):
    fs = P.ieee13_like()
    return P.BatchedGridEnvironment(fs, num_envs=num_envs, solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=EP, voltage_limits=(0.98, 1.02))


_NETS = {}


def _nets(env):
    if not _NETS:
        _NETS["pol"], _NETS["val"], _NETS["qs"] = Q._networks("ieee13", env.obs_dim, env.action_dim, [64, 64], "relu")
    return _NETS


def _make(mode, monkeypatch):
    if mode == "post":
        monkeypatch.setenv("GS_NO_FLOW2", "1")
    env = _env()
    if mode == "post":
        monkeypatch.delenv("GS_NO_FLOW2")
    kernel = env.handle.describe()["kernel"]
    assert ("flow2" in kernel) == (mode != "post"), kernel
    if mode == "mlp":
        Q._install(dict(_nets(env), env=env))
    return env


def _start(env):
    """reset, then the instances a third at a time one step apart, so that episodes of four steps end at three steps out of four"""
    env.reset(seed=RESET_SEED)
    for k in (0, 1):
        env.handle.rollout(1, "random", seed=90 + k)
        env.reset(seed=RESET_SEED + 100 * (k + 1), mask=(np.arange(env.num_envs) % 3 == k))


def _first(env, mode, T, actions=None):
    _start(env)
    rollout_device(env, T, seed=SEED, reset=False, actions=actions, policy=True if mode == "mlp" else None)


def _cont(env, mode, T, keep, **kw):
    return continue_rollout(env, T, keep, seed=SEED, policy=True if mode == "mlp" and "actions" not in kw else None, **kw)


def _entries(idx, rows):
    return sorted((int(t), int(b), np.ascontiguousarray(row).tobytes()) for (t, b), row in zip(idx, rows))


def _held(env):
    """the rollout `env` holds: the downloaded dictionary, obs_seq and the terminal list as a set"""
    d = P.download_rollout(env)
    dev = env.handle.rollout_device_arrays()
    d["obs_seq"] = dev["obs_seq"].to_host()
    d["entries"] = _entries(dev["terminal_index"].to_host(), dev["terminal_obs"].to_host())
    return d


def _slice(d, lo, hi):
    """steps lo .. hi - 1 of the held rollout `d` as a held rollout of their own"""
    out = {k: d[k][lo:hi] for k in KEYS[:5] + (("log_probs",) if "log_probs" in d else ())}
    out["obs_seq"] = d["obs_seq"][lo:hi + 1]
    out["final_observation"] = d["obs_seq"][hi]
    out["entries"] = [(t - lo, b, row) for t, b, row in d["entries"] if lo <= t < hi]
    return out


def _assert_held(env, want, tag=""):
    got = _held(env)
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in want:
        if k != "entries":
            assert _same(got[k], want[k]), (tag, k)
    assert got["entries"] == want["entries"], tag
    n = int((want["terminals"] != 0).sum())
    assert len(got["entries"]) == n == env.handle.rollout_device_view().n_terminal, tag
    # the list says what the flags and next_observations say
    for t, b, row in got["entries"]:
        assert got["terminals"][t, b] != 0 and got["next_observations"][t, b].tobytes() == row, (tag, t, b)


_CASES = {}


@pytest.fixture(scope="module")
def case():
    mp = pytest.MonkeyPatch()

    def get(mode):
        if mode not in _CASES:
            env = _make(mode, mp)
            _first(env, mode, LONG)
            long = _held(env)
            assert env.handle.rollout_window_info() == dict(T=LONG, kept=0, t0_next=LONG, T_cap=LONG)
            # episodes end in every part of the windows the tests cut: steps 1 .. 3 (dropped with keep = 3), 4 .. 6 (kept), every continue
            t_end = np.array([t for t, _, _ in long["entries"]])
            assert all(((t_end >= lo) & (t_end < hi)).any() for lo, hi in ((1, 4), (4, 7), (7, 12), (12, 17), (17, 22)))
            assert (long["terminals"] & 1).any() and ("log_probs" in long) == (mode == "mlp")
            _CASES[mode] = dict(env=env, long=long, mode=mode)
        return _CASES[mode]
    yield get
    for c in _CASES.values():
        c["env"].close()
    _CASES.clear()
    mp.undo()


# ---- 1. one continue is the tail of one long rollout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_continue_holds_the_tail_of_one_long_rollout(case, mode):
    c = case(mode)
    env, long, h = c["env"], c["long"], c["env"].handle
    for keep in (7, 6, 3, 0):                                # (6: source and destination of the shift overlap, a step at a time)
        _first(env, mode, T1)
        assert h.rollout_window_info() == dict(T=T1, kept=0, t0_next=T1, T_cap=LONG)
        v = _cont(env, mode, T2, keep, t0=T1 if keep != 3 else None)      # (None: where the first rollout's draws ended)
        assert (v.T, v.B) == (keep + T2, B)
        assert h.rollout_window_info() == dict(T=keep + T2, kept=keep, t0_next=T1 + T2, T_cap=LONG)
        _assert_held(env, _slice(long, T1 - keep, T1 + T2), (mode, keep))
    # another draw origin is another rollout
    _first(env, mode, T1)
    _cont(env, mode, T2, 3, t0=T1 + 1)
    assert not _same(_held(env)["actions"][3:], long["actions"][T1:T1 + T2]) and _same(_held(env)["actions"][:3], long["actions"][T1 - 3:T1])


# ---- 2. sliding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_three_continues_in_a_row_slide_along_the_long_rollout(case, mode):
    c = case(mode)
    env, long = c["env"], c["long"]
    _first(env, mode, T1)
    end = T1
    for k in range(3):
        kept = min(4, end)
        _cont(env, mode, T2, 4)
        end += T2
        assert env.handle.rollout_window_info() == dict(T=kept + T2, kept=kept, t0_next=end, T_cap=LONG)
        _assert_held(env, _slice(long, end - T2 - 4, end), (mode, k))
    assert end == LONG


# ---- 3. growth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_window_that_outgrows_the_capacity_carries_the_kept_part_over(case, mode, monkeypatch):
    long = case(mode)["long"]
    env = _make(mode, monkeypatch)
    try:
        h = env.handle
        _first(env, mode, T1)
        assert h.rollout_window_info()["T_cap"] == T1
        if mode == "mlp":
            P.evaluate_rollout(env, gamma=GAMMA, lam=LAM, bootstrap=3)      # (tracks sized by the old capacity are made again)
        _cont(env, mode, T2, 6)
        assert h.rollout_window_info() == dict(T=6 + T2, kept=6, t0_next=T1 + T2, T_cap=6 + T2)
        _assert_held(env, _slice(long, 1, T1 + T2), mode)
        if mode == "mlp":
            ev = P.evaluate_rollout(env, gamma=GAMMA, lam=LAM, bootstrap=3)
            assert _same(ev.log_probs.to_host(), long["log_probs"][1:T1 + T2])
        # the whole rollout kept (nothing to shift, everything to carry over), then a shift in place within the new capacity
        _cont(env, mode, T2, 6 + T2)
        assert h.rollout_window_info() == dict(T=6 + 2 * T2, kept=6 + T2, t0_next=T1 + 2 * T2, T_cap=6 + 2 * T2)
        _assert_held(env, _slice(long, 1, T1 + 2 * T2), mode)
        _cont(env, mode, T2, 2)
        assert h.rollout_window_info()["T_cap"] == 6 + 2 * T2
        _assert_held(env, _slice(long, LONG - T2 - 2, LONG), mode)
    finally:
        env.close()


def test_an_odd_batch_takes_the_narrower_paths_of_the_shift():
    """B = 5: a step of rewards is 40 bytes and a step of flags 5, so the shift moves them 8 bytes and one byte a lane (B = 70 moves
    everything but the flags 16 bytes a lane); the overlapping shift by one step and a shift by four"""
    env = _env(5)
    try:
        _first(env, "fused", T1 + T2)
        long = _held(env)
        for keep in (6, 3):
            _first(env, "fused", T1)
            _cont(env, "fused", T2, keep)
            got, want = _held(env), _slice(long, T1 - keep, T1 + T2)
            assert all(_same(got[k], want[k]) for k in want if k != "entries") and got["entries"] == want["entries"], keep
    finally:
        env.close()


# ---- 4. uploaded actions -------------------------------------------------------------------------------------------------------------
def test_uploaded_actions_cover_the_new_steps_only(case):
    c = case("fused")
    env, long = c["env"], c["long"]
    _first(env, "fused", T1, actions=long["actions"][:T1])
    _cont(env, "fused", T2, 3, actions=long["actions"][T1:T1 + T2])
    _assert_held(env, _slice(long, T1 - 3, T1 + T2))
    with pytest.raises(P.PowerFlowError):
        _cont(env, "fused", T2, 3, actions=long["actions"][:T2 + 1])      # (the shape is checked before the call)


# ---- 5. downstream -------------------------------------------------------------------------------------------------------------------
def _host(x):
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x.to_host() if hasattr(x, "to_host") else x


def _downstream(env, pol):
    h = env.handle
    dev = h.rollout_device_arrays()
    idx = dev["terminal_index"].to_host()
    order = np.argsort(idx[:, 0].astype(np.int64) * B + idx[:, 1], kind="stable")
    out = {}
    ev = P.evaluate_rollout(env, gamma=GAMMA, lam=LAM, bootstrap=3)
    out["evaluate"] = dict(values=ev.values.to_host(), terminal_values=ev.terminal_values.to_host()[order], advantages=ev.advantages.to_host(),
                           returns=ev.returns.to_host(), log_probs=ev.log_probs.to_host())
    costs = P.rollout_costs(env)
    out["costs"] = _host(dict(margins=costs.margins, counts=costs.counts, costs=costs.costs, n_violating=costs.n_violating))
    ds = P.DeviceGridDataset(env)
    out["dataset"] = {k: np.asarray(v) for k, v in ds.raw.items()}
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
    batches = OnPolicyBatches(env, 64, policy=pol, adv_norm="none", seed=5, fields=Q.FIELDS)
    batches.prepare()
    batch = next(iter(batches.epoch(0)))
    P.refresh_targets(env, batch, ("q_target", "td_value", "q_adv"), gamma=GAMMA, bootstrap=3)
    out["refreshed"] = h.rollout_q_download()
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
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and _same(x.reshape(-1), y.reshape(-1)), path


def test_every_consumer_reads_the_window_as_it_reads_the_same_arrays_loaded(case, monkeypatch):
    c = case("mlp")
    env, h, nets = c["env"], c["env"].handle, _nets(c["env"])
    _first(env, "mlp", T1)
    P.evaluate_rollout(env, gamma=GAMMA, lam=LAM, bootstrap=3)
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
    P.rollout_costs(env)
    ds = P.DeviceGridDataset(env)
    views = (h.rollout_q_arrays, h.rollout_onpolicy_arrays, h.rollout_costs_arrays, lambda: ds.sample_batch(8, seed=1))
    for view in views:
        view()
    _cont(env, "mlp", T2, 3)
    for view in views:                                          # as after any new rollout
        Q._refused(view, S, "")
    y = _make("mlp", monkeypatch)
    try:
        d = P.download_rollout(env)
        assert d["log_probs"].shape == (3 + T2, B)
        P.load_rollout_data(y, d)
        on_window, on_loaded = _downstream(env, nets["pol"]), _downstream(y, nets["pol"])
        assert np.isfinite(on_window["refreshed"]["td_target"]).all()
        _assert_same_tree(on_window, on_loaded)
    finally:
        y.close()
        Q._install(dict(nets, env=env))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def _raw(env, handle=True, **fields):
    """gs_rollout_continue through ctypes alone; returns the code"""
    h = env.handle
    cfg = _lib.gs_rollout_continue_config(ctypes.sizeof(_lib.gs_rollout_continue_config), T2, 3, _lib.POLICY["random"], SEED, T1, 0, None)
    keep = []
    for k, v in fields.items():
        if k == "actions" and v is not None:
            keep.append(np.ascontiguousarray(v, dtype=np.float64))
            v = keep[-1].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        setattr(cfg, k, v)
    return h._lib.gs_rollout_continue(h._h if handle else None, ctypes.byref(cfg))


def test_every_refusal_has_its_code_and_leaves_the_rollout_as_it_was(case, monkeypatch):
    c = case("fused")
    env, long, h = c["env"], c["long"], c["env"].handle
    _first(env, "fused", T1)
    _cont(env, "fused", T2, 3)
    before, info = _held(env), h.rollout_window_info()
    P.rollout_costs(env)

    def unchanged():
        now = _held(env)
        assert all(_same(now[k], before[k]) for k in before if k != "entries") and now["entries"] == before["entries"]
        assert h.rollout_window_info() == info
        h.rollout_costs_arrays()                                 # (what was computed over it is still current)

    assert _raw(env, handle=False) == I
    assert h._lib.gs_rollout_continue(h._h, None) == I
    for fields in (dict(struct_size=32), dict(struct_size=48), dict(T=0), dict(T=-1), dict(keep=-1), dict(keep=3 + T2 + 1), dict(policy=3), dict(policy=-1),
                   dict(policy=_lib.POLICY["uploaded"]), dict(T=2 ** 31 - 1)):
        assert _raw(env, **fields) == I, fields
        unchanged()
    assert _raw(env, policy=_lib.POLICY["mlp"]) == S            # no policy on this handle
    assert b"gs_policy_mlp_set" in h._lib.gs_last_error(h._h)
    unchanged()
    # a loaded rollout: the environment does not stand at its last slot
    P.load_rollout_data(env, {k: before[k] for k in KEYS})
    assert _raw(env) == S and b"gs_rollout_load" in h._lib.gs_last_error(h._h)
    assert all(_same(_held(env)[k], before[k]) for k in KEYS) and h.rollout_window_info() == dict(T=3 + T2, kept=0, t0_next=3 + T2, T_cap=LONG)
    # ... and keep = 0 goes on from where the environment stands, as gs_rollout would
    _cont(env, "fused", T2, 0, t0=T1 + T2)
    _assert_held(env, _slice(long, T1 + T2, T1 + 2 * T2))
    # the environment moved since the rollout ended
    before, info = _held(env), h.rollout_window_info()
    env.step(np.zeros((B, env.action_dim)))
    assert _raw(env, keep=1) == S and b"moved" in h._lib.gs_last_error(h._h)
    now = _held(env)
    assert all(_same(now[k], before[k]) for k in before if k != "entries") and now["entries"] == before["entries"] and h.rollout_window_info() == info
    assert _raw(env, keep=0) == _lib.GS_OK and h.rollout_window_info()["kept"] == 0
    h.synchronize()
    # no rollout on the handle
    e = _make("fused", monkeypatch)
    try:
        e.reset(seed=RESET_SEED)
        assert _raw(e, keep=1) == S and b"no rollout" in e.handle._lib.gs_last_error(e.handle._h)
        assert e.handle.rollout_window_info() == dict(T=0, kept=0, t0_next=0, T_cap=0)
        _start(e)
        assert _raw(e, keep=0, t0=0) == _lib.GS_OK
        e.handle._rollout_T = T2
        assert _same(P.download_rollout(e)["observations"], long["observations"][:T2])
    finally:
        e.close()


# ---- 7. episodes ---------------------------------------------------------------------------------------------------------------------
def test_episode_accounting_refuses_to_continue_over_kept_steps_and_counts_the_window_fresh(case):
    c = case("fused")
    env = c["env"]
    _first(env, "fused", T1)
    rollout_episodes(env, start="fresh")
    _cont(env, "fused", T2, 3)
    Q._refused(lambda: rollout_episodes(env, start="continue"), S, "window")
    d = env.handle.rollout_download(("rewards", "terminals"))
    rec, stats, carry = episodes_np(d["rewards"], d["terminals"], start="fresh")
    view = rollout_episodes(env, start="fresh")
    got = view.download()
    assert got["n_episodes"] == len(rec["episode_return"]) == d["n_terminal"] > 0
    for k in ("episode_index", "episode_return", "episode_length", "episode_ordinal", "episode_flags"):
        assert _same(got[k], rec[k]), k
    for k in ("ep_return", "ep_length", "ep_ordinal"):
        assert _same(got[k], carry[k]), k
    assert view.stats.count == stats.count
    # without kept steps a continue may be accounted on
    _first(env, "fused", T1)
    rollout_episodes(env, start="fresh")
    _cont(env, "fused", T2, 0)
    assert rollout_episodes(env, start="continue").n_episodes == int((env.handle.rollout_download(("terminals",))["terminals"] != 0).sum())
