"""CPU: per-minibatch targets (include/gridstep.h "per-minibatch targets") -- ``refresh_rows_np`` against a plain
loop, the existing arithmetic restatements restricted to the rows of a batch against their full-array results, the config struct,
every ``ValueError``, and ``DeviceLearner(fresh_targets=...)`` on a recording handle: the default calls no new entry, and
``fresh_targets=True`` issues the refreshes in the reference's order (algorithms/offline.py:166-255 for the policy-action wiring,
:482-540 for IQL's)."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import DeviceLearner
from grid_fed_rl_gym_amd.rollout import q_combine_np, refresh_rows_np, refresh_targets, td_policy_np, td_target_np

T, B = 7, 5
N = T * B


def _dataset(seed=0):
    rng = np.random.default_rng(seed)
    flags = rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=(T, B))
    flags[2, 3], flags[4, 0], flags[0, 1] = 1, 2, 0            # (both kinds and a live transition, whatever the draw)
    tb = np.argwhere(flags != 0)
    tb = tb[rng.permutation(len(tb))].astype(np.int32)           # the terminal list is appended in no particular order
    return rng, flags, tb


def _loop(indices, flags, tb, mask):
    own, nxt, pairs = [], [], []
    for i, j in enumerate(indices):
        j = min(max(int(j), 0), N - 1)
        own.append(j); nxt.append(j + B)
        t, b = divmod(j, B)
        if flags[t, b] & mask:
            for e in range(len(tb)):
                if tb[e, 0] == t and tb[e, 1] == b:
                    pairs.append((i, e))
    return np.array(own), np.array(nxt), np.array(pairs, dtype=np.int64).reshape(-1, 2)


def _lists(rng, flags):
    ended = np.nonzero(flags.reshape(-1) != 0)[0]
    live = np.nonzero(flags.reshape(-1) == 0)[0]
    perm = rng.permutation(N)
    return {"one": perm[:1], "some": perm[:13], "all": perm, "twice": np.concatenate([perm, perm[::-1]]), "terminal only": rng.permutation(ended),
            "no terminal": rng.permutation(live), "outside": np.array([-3, N + 4, 2, N - 1, 0])}


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_refresh_rows_np_against_a_plain_loop(mask):
    rng, flags, tb = _dataset()
    assert (flags == 1).any() and (flags == 2).any()
    for name, idx in _lists(rng, flags).items():
        own, nxt, pairs = refresh_rows_np(idx, T, B, flags, tb, mask)
        w_own, w_nxt, w_pairs = _loop(idx, flags, tb, mask)
        assert np.array_equal(own, w_own) and np.array_equal(nxt, w_nxt) and np.array_equal(pairs, w_pairs), (name, mask)
        assert pairs.shape == (len(w_pairs), 2) and (np.diff(pairs[:, 0]) > 0).all()      # ascending i
        if name == "no terminal" or mask == 0:
            assert len(pairs) == 0
        if name == "terminal only" and mask == 3:
            assert np.array_equal(pairs[:, 0], np.arange(len(idx))) and len(idx) == len(tb)
        if name == "twice" and mask == 3:
            assert len(pairs) == 2 * len(tb)            # a duplicate index once per occurrence
    # a terminal list shorter than the flags (a full list's tail): the rows without an entry are not pairs
    _, _, pairs = refresh_rows_np(np.arange(N), T, B, flags, tb[:2], 3)
    assert len(pairs) == 2 and set(pairs[:, 1]) == {0, 1}


def _restrict(x, rows):
    return np.asarray(x).reshape(N, *np.shape(x)[2:])[rows][None]      # [1, n, ...]: one step of n instances


@pytest.mark.parametrize("mask", [0, 1, 3])
def test_the_arithmetic_restatements_on_the_rows_of_a_batch_are_the_full_arrays_rows(mask):
    """What the refresh writes at the rows of a batch IS the full evaluation's value there: td_policy_np, td_target_np and
    q_combine_np applied to the batch's rows alone (as one step of n instances, the terminal entries re-indexed through the (i, e)
    pairs) equal their full-array results at those rows, bit for bit."""
    rng, flags, tb = _dataset(1)
    rew, lp, q0, q1 = (rng.normal(size=(T, B)) for _ in range(4))
    values = rng.normal(size=(T + 1, B))
    t_q, t_lp, t_v = (rng.normal(size=len(tb)) for _ in range(3))
    gamma, alpha = 0.97, 0.2
    qmin_on, qmin_tg, adv = q_combine_np([q0, q1], [q1, q0], values)
    full_pol = td_policy_np(rew, lp, qmin_on, flags, t_q, tb, gamma, alpha, mask, 0.5, 0.25, terminal_log_probs=t_lp)
    full_val = td_target_np(rew, values, flags, t_v, tb, gamma, mask, 0.5, 0.25)
    for name, idx in _lists(rng, flags).items():
        own, nxt, pairs = refresh_rows_np(idx, T, B, flags, tb, mask)
        n = len(idx)
        sub_tb = np.stack([np.zeros(len(pairs), dtype=np.int64), pairs[:, 0]], axis=1)
        r = lambda x: _restrict(x, own)
        got = td_policy_np(r(rew), r(lp), r(qmin_on), r(flags), t_q[pairs[:, 1]], sub_tb, gamma, alpha, mask, 0.5, 0.25, terminal_log_probs=t_lp[pairs[:, 1]])
        assert np.array_equal(got[0], full_pol.reshape(-1)[own]), (name, mask)
        sub_values = np.stack([values.reshape(-1)[own], values.reshape(-1)[nxt]])      # [2, n]: V(s_j), V(next state of j)
        got = td_target_np(r(rew), sub_values, r(flags), t_v[pairs[:, 1]], sub_tb, gamma, mask, 0.5, 0.25)
        assert np.array_equal(got[0], full_val.reshape(-1)[own]), (name, mask)
        a, b, c = q_combine_np([r(q0), r(q1)], [r(q1), r(q0)], r(values[:T]))
        assert np.array_equal(a[0], qmin_on.reshape(-1)[own]) and np.array_equal(b[0], qmin_tg.reshape(-1)[own]) and np.array_equal(c[0], adv.reshape(-1)[own])
        assert got.shape == (1, n)


def test_the_config_struct_is_the_headers():
    assert ctypes.sizeof(_lib.gs_refresh_config) == 72 and ctypes.sizeof(_lib.gs_refresh_config) % 8 == 0
    cfg = _lib.refresh_config(("td_policy", "q_adv"), 0.97, 0.2, 3, False, (1 << 64) - 1, 5, 0.5, 0.25)
    assert (cfg.struct_size, cfg.groups, cfg.bootstrap_mask, cfg.stochastic, cfg.gamma, cfg.alpha, cfg.reward_shift, cfg.reward_scale, cfg.seed, cfg.draw,
            cfg.reserved, cfg.reserved2) == (72, 9, 3, 0, 0.97, 0.2, 0.5, 0.25, (1 << 64) - 1, 5, 0, 0)
    assert (_lib.GS_REFRESH_TD_POLICY, _lib.GS_REFRESH_Q_TARGET, _lib.GS_REFRESH_TD_VALUE, _lib.GS_REFRESH_Q_ADV) == (1, 2, 4, 8)
    assert _lib.refresh_groups("td_value") == 4 and _lib.refresh_groups(["q_target", "td_value"]) == 6 and _lib.refresh_groups(15) == 15
    assert "gs_learner_refresh" in [s[0] for s in _lib.SYMBOLS]


def test_the_host_checks_of_the_entry_in_a_program_of_their_own(tmp_path):
    """tests/native/refresh_check_host.cpp: the GS_E_INVALID rules and the scratch sizes of csrc/refresh.h, with no device and no
    Python in the process (the form in which they are also run under a sanitizer)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "grid_fed_rl_gym_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "refresh_check_host"
    subprocess.run([hipcc, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-I", csrc, "-x", "c++", os.path.join(root, "tests", "native", "refresh_check_host.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["checks: ok", "sizes: ok", "clamp: ok"], r.stdout + r.stderr


# ---- host logic on a recording handle (no device) ----
class _Handle:
    def __init__(self, steps=None):
        self.calls, self.steps = [], dict(steps or {})

    def learner_create(self, net, cfg):
        self.calls.append(("create", net))

    def learner_set_loss(self, net, loss):
        self.calls.append(("loss", net, int(loss.kind)))

    def learner_set_signal(self, net, signal):
        self.calls.append(("signal", net, signal))

    def q_set_target_source(self, source):
        self.calls.append(("q_target", source))

    def learner_info(self, net):
        return dict(step=self.steps.get(net, 0))

    def learner_step(self, net, batch, n, stream=None):
        self.calls.append(("step", net))
        self.steps[net] = self.steps.get(net, 0) + 1

    def learner_step_pathwise(self, batch, n, cfg, stream=None):
        self.calls.append(("pathwise", 0))
        self.steps[0] = self.steps.get(0, 0) + 1

    def learner_step_conservative(self, net, batch, n, cfg, stream=None):
        self.calls.append(("conservative", net, int(cfg.draw)))
        self.steps[net] = self.steps.get(net, 0) + 1

    def learner_refresh(self, batch, cfg, n=None, stream=None):
        self.calls.append(("refresh", int(cfg.groups), int(cfg.draw), int(cfg.bootstrap_mask), cfg.gamma, cfg.alpha, int(cfg.stochastic), int(cfg.seed)))


class _Env:
    def __init__(self, steps=None):
        self.handle = _Handle(steps)


class _Batch(dict):
    pass


def _batch(n=4):
    return _Batch(observations=np.zeros((n, 3), dtype=np.float32), indices=np.zeros(n, dtype=np.int32))


def test_the_default_learner_calls_no_new_entry():
    for kw in (dict(nets=("policy", "q1", "q2"), policy_loss="pathwise", q_target="policy", conservative_weight=5.0),
               dict(nets=("policy", "value", "q1", "q2"), policy_loss="awr", value_loss="expectile", advantage_source="q", value_target="q"),
               dict(nets=("policy", "value"))):
        env = _Env()
        learner = DeviceLearner(env, **kw)
        assert learner.fresh_targets is False
        for _ in range(2):
            learner.step(_batch())
        assert not [c for c in env.handle.calls if c[0] == "refresh"], kw
        assert len([c for c in env.handle.calls if c[0] in ("step", "pathwise", "conservative")]) == 2 * len(kw["nets"])


def test_fresh_targets_issues_the_refreshes_in_the_references_order():
    # the policy-action wiring (CQL / TD3 + BC): TD_POLICY, the Q steps, the actor; draw = the first Q net's steps taken
    env = _Env(steps={5: 7, 6: 7})
    learner = DeviceLearner(env, nets=("policy", "q1", "q2"), policy_loss="pathwise", alpha=0.2, q_target="policy", conservative_weight=5.0, fresh_targets=True,
                            gamma=0.97, bootstrap=("terminated", "truncated"), target_seed=11)
    env.handle.calls.clear()
    learner.step(_batch())
    learner.step(_batch())
    P_ = _lib.GS_REFRESH_TD_POLICY
    assert env.handle.calls == [("refresh", P_, 7, 3, 0.97, 0.2, 1, 11), ("conservative", 5, 7), ("conservative", 6, 7), ("pathwise", 0),
                                ("refresh", P_, 8, 3, 0.97, 0.2, 1, 11), ("conservative", 5, 8), ("conservative", 6, 8), ("pathwise", 0)]
    # without the conservative penalty and with the deterministic actor: plain Q steps, stochastic = 0
    env = _Env()
    learner = DeviceLearner(env, nets=("q2", "policy"), policy_loss="pathwise", pathwise_stochastic=False, q_target="policy", fresh_targets=True)
    env.handle.calls.clear()
    learner.step(_batch())
    assert env.handle.calls == [("refresh", P_, 0, 0, 0.99, 0.0, 0, 0), ("step", 6), ("pathwise", 0)]
    # the IQL wiring: Q_TARGET, the value step, TD_VALUE, the Q steps, Q_ADV, the policy step
    env = _Env()
    learner = DeviceLearner(env, nets=("policy", "value", "q1", "q2"), policy_loss="awr", value_loss="expectile", advantage_source="q", value_target="q",
                            fresh_targets=True, gamma=0.9, bootstrap="truncated")
    env.handle.calls.clear()
    learner.step(_batch())
    G = lambda bits: ("refresh", bits, 0, 2, 0.9, 0.0, 1, 0)
    assert env.handle.calls == [G(_lib.GS_REFRESH_Q_TARGET), ("step", 1), G(_lib.GS_REFRESH_TD_VALUE), ("step", 5), ("step", 6), G(_lib.GS_REFRESH_Q_ADV),
                                ("step", 0)]


@pytest.mark.parametrize("kw", [dict(nets=("policy", "value"), fresh_targets=True),
                                dict(nets=("policy", "value"), advantage_source="q", value_target="q", fresh_targets=True),
                                dict(nets=("q1", "q2"), fresh_targets=True),                              # neither wiring
                                dict(nets=("policy", "value", "q1"), advantage_source="q", fresh_targets=True),
                                dict(nets=("q1",), q_target="policy", fresh_targets=1),
                                dict(nets=("q1",), q_target="policy", fresh_targets=True, gamma=math.nan),
                                dict(nets=("q1",), q_target="policy", fresh_targets=True, bootstrap=("ended",)),
                                dict(nets=("q1",), q_target="policy", fresh_targets=True, target_seed=-1),
                                dict(nets=("q1",), q_target="policy", fresh_targets=True, target_seed=1.5)])
def test_device_learner_refuses_fresh_targets_before_anything_is_created(kw):
    env = _Env()
    with pytest.raises(ValueError):
        DeviceLearner(env, **kw)
    assert env.handle.calls == []


def test_every_value_error_of_the_new_functions():
    _, flags, tb = _dataset()
    ok = np.arange(4)
    for bad in (lambda: refresh_rows_np(np.zeros((2, 2), dtype=np.int64), T, B, flags, tb, 0), lambda: refresh_rows_np(np.array([0.5, 1.0]), T, B, flags, tb, 0),
                lambda: refresh_rows_np(ok, 0, B, flags, tb, 0), lambda: refresh_rows_np(ok, T, 0, flags, tb, 0), lambda: refresh_rows_np(ok, T, B, flags, tb, 4),
                lambda: refresh_rows_np(ok, T, B, flags, tb, -1), lambda: refresh_rows_np(ok, T, B, flags[:-1], tb, 0),
                lambda: _lib.refresh_groups("td"), lambda: _lib.refresh_groups(["q_adv", "next"])):
        with pytest.raises(ValueError):
            bad()
    env = _Env()
    b = _batch()
    for kw in (dict(groups=()), dict(groups=0), dict(groups=16), dict(groups="values"), dict(groups="td_policy", alpha=-1.0), dict(groups="td_policy", alpha=math.nan),
               dict(groups="td_policy", alpha=math.inf), dict(groups="td_policy", stochastic=1), dict(groups="td_policy", seed=-1), dict(groups="td_policy", seed=1 << 64),
               dict(groups="td_policy", draw=1 << 32), dict(groups="td_policy", draw=True), dict(groups="q_adv", bootstrap=("ended",))):
        with pytest.raises(ValueError):
            refresh_targets(env, b, **kw)
    for batch in ({}, dict(indices=None), None):
        with pytest.raises(ValueError):
            refresh_targets(env, batch, "q_adv")
    assert env.handle.calls == []
    refresh_targets(env, b, ("q_target", "td_value"), gamma=0.9, bootstrap=3, seed=5, draw=2)
    assert env.handle.calls == [("refresh", 6, 2, 3, 0.9, 0.0, 1, 5)]
