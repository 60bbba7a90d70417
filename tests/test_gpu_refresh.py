"""GPU: per-minibatch targets (include/gridstep.h "per-minibatch targets") -- ``gs_learner_refresh`` against the
parent's own entries.  A refresh of the list L leaves, at the rows of L and at the terminal entries reached from L, exactly the bits a
full ``gs_rollout_evaluate_q_next`` / ``gs_rollout_evaluate_q`` under the same config and images leaves there, and every other row and
entry keeps the bits it had (compared with a download taken just before the refresh).

The fixtures, recipe and bounds are those of tests/test_gpu_q_next.py (imported, not edited): 13-bus T = 37, B = 5 (185 rows in tiles of
64, 64, 57; ``episode_length`` 14: both terminal kinds, asserted), 123-bus T = 3, B = 70 (three observation panels), the 40-bus
synthetic feeder (81 terminal rows among 162), a tanh and a single-layer case.  Index lists: n = 1, 33, 64, 65 of ``permutation_np``,
all rows permuted, every index twice, terminal transitions only, none of them; masks 0 and 3.

Bounds, none computed from the device: everything is bit-equal, except the noise, which lies within 1e-9 of ``q_next_noise_np`` (the
project's bound: the host's log, sin and cos are a library's).  No check is vacuous: for every list the fresh values differ from the
stale ones somewhere on the list (asserted).

What the scratch of a refresh holds (the (i, e) list, the gathered rows) has no view of its own in the ABI; ``refresh_rows_np`` is
checked through what it implies: which rows and which terminal entries change, and to which bits."""
import ctypes as C
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, permutation_np, q_next_noise_np, refresh_rows_np, refresh_targets, rollout_device, td_policy_np, td_target_np
from tests import test_gpu_q_next as TQ

pytestmark = pytest.mark.gpu

GAMMA, ALPHA, SEED = TQ.GAMMA, TQ.ALPHA, TQ.SEED
STALE, FRESH = 9, 4                # the draw the arrays are left under before a refresh, and the refresh's
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
_same, _install = TQ._same, TQ._install

ROW_KEYS = {
    "td_policy": ("next_pre_head", "next_actions", "next_noise", "next_log_probs", "q_next0", "q_next1", "q_next_min", "td_target"),
    "q_target": ("q_target0", "q_target1", "q_min_target"),
    "td_value": ("td_value",),
    "q_adv": ("q_online0", "q_online1", "q_min_online", "q_adv"),
}
TERM_KEYS = ("term_pre_head", "term_actions", "term_noise", "term_log_probs", "term_q0", "term_q1", "term_q_min", "term_value")
ALL = ("td_policy", "q_target", "td_value", "q_adv")

_PREPARED, _BUFFERS = {}, []


@pytest.fixture(scope="module")
def prepared():
    def get(name):
        if name not in _PREPARED:
            _PREPARED[name] = TQ._build(name)
        return _PREPARED[name]
    yield get
    for c in _PREPARED.values():
        c["env"].close()
        if "twin" in c:
            c["twin"][0].close()
    _PREPARED.clear()
    hip = _lib._hip_runtime()
    for p in _BUFFERS:
        hip.hipFree(p)
    _BUFFERS.clear()


def _dev(idx):
    """a batch that holds nothing but these indices, in device memory of the test's own"""
    a = np.ascontiguousarray(idx, dtype=np.int32)
    hip = _lib._hip_runtime()
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 4))) == 0 and p.value
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0      # hipMemcpyHostToDevice
    _BUFFERS.append(p)
    return dict(indices=_lib.DeviceArray(p.value, a.shape, "<i4"))


def _twin_of(c):
    if "twin" not in c:
        c["twin"] = TQ._twin(c)
        assert _same(c["twin"][1]["observations"], c["data"]["observations"]) and _same(c["twin"][1]["rewards"], c["data"]["rewards"])
    return c["twin"]


def _snap(env, q_next=True, q=True):
    """every array of both views, by one flat name each"""
    h, out = env.handle, {}
    if q_next:
        for k, v in h.rollout_q_next_download().items():
            if isinstance(v, list):
                for w, x in enumerate(v):
                    out[f"{k}{w}"] = x
            else:
                out[k] = v
    if q:
        d = h.rollout_q_download()
        for src in ("online", "target"):
            out[f"q_min_{src}"] = d["q_min"][src]
            for w in range(2):
                out[f"q_{src}{w}"] = d["q"][src][w]
        out["q_adv"], out["td_value"] = d["q_adv"], d["td_target"]
    return out


def _lists(c, names=None):
    T, B, flags = c["T"], c["B"], c["data"]["terminals"].reshape(-1)
    N = T * B
    perm = permutation_np(5, 3, N)
    rng = np.random.default_rng(2)
    ended, live = np.nonzero(flags != 0)[0], np.nonzero(flags == 0)[0]
    assert len(ended) and len(live)
    every = {"n=1": perm[:1], "n=33": perm[:33], "n=64": perm[:64], "n=65": perm[:65], "all": perm, "twice": np.concatenate([perm, perm[::-1]]),
             "terminal": rng.permutation(ended), "live": rng.permutation(live)}
    return {k: every[k] for k in (names or every)}


def _evaluate_all(env, mask, draw):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=mask)
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=mask)
    P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=ALPHA, bootstrap=mask, stochastic=True, seed=SEED, draw=draw)


def _check(c, idx, mask, groups, before, after, fresh, fresh_data=None, tag="", constant=()):
    """at the rows of ``idx`` and the terminal entries reached from them ``after`` holds ``fresh``'s bits, elsewhere ``before``'s; and
    the refresh was not vacuous: every group's fresh values differ from the stale ones somewhere on the list -- but for the groups
    in ``constant``, whose values on this list do not depend on the images (asserted to be the stale bits)"""
    d, T, B = c["data"], c["T"], c["B"]
    N = T * B
    own, nxt, pairs = refresh_rows_np(idx, T, B, d["terminals"], d["terminal_index"], mask)
    assert np.array_equal(nxt, own + B)
    on = np.zeros(N, dtype=bool)
    on[own] = True
    flat = lambda x: x.reshape(N, -1)
    for g in ALL:
        moved = False
        for k in ROW_KEYS[g]:
            if k not in before:
                continue
            b, a, f = flat(before[k]), flat(after[k]), flat(fresh[k])
            if g in groups:
                assert _same(a[on], f[on]), (tag, k, "the rows of the list hold the full evaluation's bits")
                assert _same(a[~on], b[~on]), (tag, k, "every other row keeps its bits")
                moved |= not np.array_equal(f[on], b[on])
            else:
                assert _same(a, b), (tag, k, "a group that was not asked for is not written")
        if g in groups:
            assert moved != (g in constant), (tag, g, "the fresh values differ from the stale ones somewhere on the list")
    # terminal entries: reached from the list under the mask; entry by entry through (t, b) where `fresh` comes from another handle
    ti = d["terminal_index"]
    hit = np.zeros(len(ti), dtype=bool)
    hit[pairs[:, 1]] = True
    if fresh_data is None:
        src = np.arange(len(ti))
    else:
        where = {(int(t), int(b)): e for e, (t, b) in enumerate(fresh_data["terminal_index"])}
        src = np.array([where[(int(t), int(b))] for t, b in ti], dtype=np.int64)
    reached = "td_policy" in groups and mask != 0
    for k in TERM_KEYS:
        if k not in before:
            continue
        b, a, f = before[k], after[k], fresh[k][src]
        if reached:
            assert _same(a[hit], f[hit]), (tag, k, "the terminal entries reached from the list")
            assert _same(a[~hit], b[~hit]), (tag, k, "every other terminal entry keeps its bits")
        else:
            assert _same(a, b), (tag, k)
    want_pairs = [(i, e) for i, j in enumerate(own) if d["terminals"].reshape(-1)[j] & mask for e in np.nonzero((ti[:, 0].astype(np.int64) * B + ti[:, 1]) == j)[0]]
    assert [tuple(p) for p in pairs] == want_pairs
    return own, pairs


def _restatements(c, idx, mask, after, own, pairs):
    """td_target, q_next_min, term_value and the noise at the refreshed rows against the NumPy restatements fed the device's arrays"""
    d, T, B = c["data"], c["T"], c["B"]
    A = c["env"].action_dim
    eps = after["next_noise"].reshape(T * B, A)[own]
    assert TQ._err(eps, q_next_noise_np(SEED, FRESH, own, A)) <= 1e-9 and np.abs(eps).max() > 0.0
    want = td_policy_np(d["rewards"], after["next_log_probs"], after["q_next_min"], d["terminals"], after["term_q_min"] if mask else [],
                        d["terminal_index"] if mask else np.zeros((0, 2)), GAMMA, ALPHA, mask, terminal_log_probs=after["term_log_probs"] if mask else None)
    assert _same(after["td_target"].reshape(-1)[own], want.reshape(-1)[own])
    assert _same(after["q_next_min"].reshape(-1)[own], np.fmin(after["q_next0"], after["q_next1"]).reshape(-1)[own])
    if mask and len(pairs):
        e = pairs[:, 1]
        ti = d["terminal_index"][e]
        assert TQ._err(after["term_noise"][e], q_next_noise_np(SEED, FRESH, ti[:, 0].astype(np.int64) * B + ti[:, 1], A, terminal=True)) <= 1e-9
        assert _same(after["term_q_min"][e], np.fmin(after["term_q0"], after["term_q1"])[e])
        assert _same(after["term_value"][e], (after["term_q_min"] - ALPHA * after["term_log_probs"])[e])


CASE_LISTS = {"ieee13-relu": None, "ieee123-relu": ("n=33", "all", "terminal"), "scal40-relu": ("n=65", "all", "terminal"), "ieee13-tanh40": ("n=33", "twice"),
              "ieee13-single": ("n=64", "live")}


@pytest.mark.parametrize("mask", [0, 3])
@pytest.mark.parametrize("name", list(CASE_LISTS))
def test_a_refresh_leaves_the_full_evaluations_bits_on_the_list_and_nothing_else(prepared, name, mask):
    """GS_REFRESH_TD_POLICY under unchanged images: the arrays are left under draw STALE, the list is refreshed under draw FRESH and
    compared with the SAME handle's full evaluation under draw FRESH."""
    c = prepared(name)
    env, d = c["env"], c["data"]
    if name == "ieee13-relu":
        assert (d["terminals"] == 1).any() and ((d["terminals"] & 2) != 0).any(), "both terminal kinds occur"
    if name == "scal40-relu":
        assert (d["terminals"] != 0).sum() >= 81 and d["terminals"].size == 162
    _install(c)
    _evaluate_all(env, mask, FRESH)
    fresh = _snap(env)
    for tag, idx in _lists(c, CASE_LISTS[name]).items():
        _evaluate_all(env, mask, STALE)
        before = _snap(env)
        refresh_targets(env, _dev(idx), "td_policy", gamma=GAMMA, alpha=ALPHA, bootstrap=mask, seed=SEED, draw=FRESH)
        after = _snap(env)
        own, pairs = _check(c, idx, mask, ("td_policy",), before, after, fresh, tag=(name, mask, tag))
        _restatements(c, idx, mask, after, own, pairs)
        if tag == "terminal":
            assert (len(pairs) == len(idx)) == (mask == 3)
        if tag == "live":
            assert len(pairs) == 0


def _learner(env, **kw):
    return P.DeviceLearner(env, nets=("q1", "q2", "policy", "value"), **TQ.HYPER, policy_loss="pathwise", alpha=ALPHA, bc_coef=2.5, pathwise_seed=11,
                           q_target="policy", conservative_weight=1.0, conservative_seed=13, **kw)


def _fresh_full(c, learner, mask):
    """the full evaluations on a second handle on which the learner's CURRENT networks were installed: the policy, the value network,
    the TARGET twins (as online networks: q[target], td_target of the policy, the terminal arrays) and then the ONLINE twins"""
    twin, d2 = _twin_of(c)
    online, target = [learner.q(w) for w in range(2)], [learner.target_q(w) for w in range(2)]
    twin.set_policy(learner.policy(), stochastic=True)
    twin.set_value(learner.value())
    for w in range(2):
        twin.set_q(w, target[w])
    _evaluate_all(twin, mask, FRESH)
    fresh = _snap(twin)
    for w in range(2):
        twin.set_q(w, online[w])
    P.evaluate_rollout_q(twin, gamma=GAMMA, bootstrap=mask)
    on = _snap(twin, q_next=False)
    for k in ROW_KEYS["q_adv"]:
        fresh[k] = on[k]
    values = twin.handle.rollout_onpolicy_download(("values", "terminal_values"))
    return fresh, d2, values


MOVED_LISTS = {"ieee13-relu": ("n=1", "n=33", "n=65", "twice", "terminal"), "ieee123-relu": ("all",), "scal40-relu": ("n=65",), "ieee13-tanh40": ("n=64",),
               "ieee13-single": ("live",)}


@pytest.mark.parametrize("mask", [0, 3])
@pytest.mark.parametrize("name", list(MOVED_LISTS))
def test_a_refresh_sees_the_current_images(prepared, name, mask):
    """One conservative Q step per twin, one pathwise actor step, one value step and ``update_targets`` move every image; a refresh
    of all four groups then equals, on the list, the full evaluations of a second handle with ``learner.policy()``,
    ``learner.value()``, ``learner.q(w)`` and ``learner.target_q(w)`` installed.  Before each list the images move again, so the
    rows an earlier list refreshed are stale once more."""
    c = prepared(name)
    env, d, T, B = c["env"], c["data"], c["T"], c["B"]
    h = env.handle
    _install(c)
    _evaluate_all(env, mask, STALE)
    learner = _learner(env)
    for s, (tag, idx) in enumerate(_lists(c, MOVED_LISTS[name]).items()):
        learner.step(h.onpolicy_batch(5, 50 + s, 0, min(64, T * B)))
        learner.update_targets(0.5)
        P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=ALPHA, bootstrap=mask, stochastic=True, seed=SEED, draw=STALE)
        before = _snap(env)
        fresh, d2, values = _fresh_full(c, learner, mask)
        batch = _dev(idx)
        if s % 2 == 0:            # the four groups in one call, or one call each
            refresh_targets(env, batch, ALL, gamma=GAMMA, alpha=ALPHA, bootstrap=mask, seed=SEED, draw=FRESH)
        else:
            for g in ALL:
                refresh_targets(env, batch, g, gamma=GAMMA, alpha=ALPHA, bootstrap=mask, seed=SEED, draw=FRESH)
        after = _snap(env)
        # (under mask 0 the target of a transition that ended an episode is r' alone, whatever the networks and the noise: on the
        # terminal-only list neither td_value nor td_target can move, which is asserted in place of the opposite; the group
        # "td_policy" still moves there through its other arrays)
        fixed = mask == 0 and tag == "terminal"
        own, pairs = _check(c, idx, mask, ALL, before, after, fresh, fresh_data=d2, tag=(name, mask, tag), constant=("td_value",) if fixed else ())
        _restatements(c, idx, mask, after, own, pairs)
        for k in ("td_target", "td_value", "q_min_target", "q_adv"):      # each signal a step reads moved with the images
            moved = not np.array_equal(fresh[k].reshape(-1)[own], before[k].reshape(-1)[own])
            assert moved != (fixed and k in ("td_target", "td_value")), (tag, k)
        # td (IQL's target) and q_adv against the restatements fed the second handle's values of the current value network
        where = {(int(t), int(b)): e for e, (t, b) in enumerate(d2["terminal_index"])}
        tv = np.array([values["terminal_values"][where[(int(t), int(b))]] for t, b in d["terminal_index"]])
        want = td_target_np(d["rewards"], values["values"], d["terminals"], tv, d["terminal_index"], GAMMA, mask)
        assert _same(after["td_value"].reshape(-1)[own], want.reshape(-1)[own])
        assert _same(after["q_adv"].reshape(-1)[own], (after["q_min_online"] - values["values"][:T]).reshape(-1)[own])
        assert _same(after["q_min_target"].reshape(-1)[own], np.fmin(after["q_target0"], after["q_target1"]).reshape(-1)[own])
    learner.set_q_target("value")
    _install(c)


def _state(learner, nets):
    out = {net: learner.download(net, ("params", "grads", "m", "v")) for net in nets}
    for net in nets:
        out[net]["stats"] = learner.stats(net)
    for w, net in enumerate(("q1", "q2")):
        if net in nets:
            out[net]["target"] = learner.env.handle.q_target_download(w, learner.info(net)["param_count"])
    return out


def _assert_same_state(a, b):
    for net in a:
        for k, x in a[net].items():
            if k == "stats":
                for s, v in x.items():
                    w = b[net][k][s]
                    assert v == w or (isinstance(v, float) and math.isnan(v) and math.isnan(w)), (net, s, v, w)
            else:
                assert _same(x, b[net][k]), (net, k)


@pytest.mark.parametrize("wiring", ["policy", "iql"])
def test_the_fresh_learner_is_the_manual_sequence_of_refreshes_and_steps(prepared, wiring):
    """``DeviceLearner(fresh_targets=True).step(batch)`` over three minibatches against ``refresh_targets`` and the parent's steps
    issued by hand on a second handle: parameters, Adam's moments, gradients, target images and ``stats``, bit for bit."""
    c = prepared("ieee13-relu")
    env, mask = c["env"], 3
    twin, _ = _twin_of(c)
    if wiring == "policy":
        nets = ("q1", "q2", "policy")
        kw = dict(nets=nets, **TQ.HYPER, policy_loss="pathwise", alpha=ALPHA, bc_coef=2.5, pathwise_seed=11, q_target="policy", conservative_weight=1.0,
                  conservative_seed=13)
    else:
        nets = ("policy", "value", "q1", "q2")
        kw = dict(nets=nets, **TQ.HYPER, policy_loss="awr", temperature=3.0, weight_max=100.0, value_loss="expectile", expectile=0.7, advantage_source="q",
                  value_target="q")
    states = []
    for e, fresh in ((env, True), (twin, False)):
        _install(dict(c, env=e))
        _evaluate_all(e, mask, STALE)
        OnPolicyBatches(e, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=TQ.FIELDS).prepare()
        learner = P.DeviceLearner(e, **kw, **(dict(fresh_targets=True, gamma=GAMMA, bootstrap=mask, target_seed=SEED) if fresh else {}))
        h = e.handle
        td0 = _snap(e)
        for s, n in enumerate((33, 64, 65)):
            batch = h.onpolicy_batch(5, s, 0, n)
            if fresh:
                learner.step(batch)
            elif wiring == "policy":
                refresh_targets(e, batch, "td_policy", gamma=GAMMA, alpha=ALPHA, bootstrap=mask, seed=SEED, draw=learner.info("q1")["step"])
                assert learner.info("q1")["step"] == s
                learner.step(batch)            # the parent's order: q1, q2 (conservative), the pathwise actor
            else:
                r = lambda g: refresh_targets(e, batch, g, gamma=GAMMA, bootstrap=mask, seed=SEED)
                r("q_target"); h.learner_step("value", batch, n)
                r("td_value"); h.learner_step("q1", batch, n); h.learner_step("q2", batch, n)
                r("q_adv"); h.learner_step("policy", batch, n)
            learner.update_targets(0.25)
        states.append((_state(learner, nets), _snap(e)))
        key = "td_target" if wiring == "policy" else "q_adv"
        assert not np.array_equal(states[-1][1][key], td0[key]), "the steps read refreshed signals"
        learner.set_q_target("value")
    _assert_same_state(states[0][0], states[1][0])
    for k, x in states[0][1].items():
        if not k.startswith("term_"):          # (the terminal lists of two handles are in no particular order)
            assert _same(x, states[1][1][k]), k
    _install(c)
    _install(dict(c, env=twin))


def test_after_refreshes_the_default_learner_is_a_handle_that_never_refreshed(prepared):
    c = prepared("ieee13-relu")
    env = c["env"]
    _install(c)
    _evaluate_all(env, 3, STALE)
    refresh_targets(env, _dev(_lists(c, ("n=65",))["n=65"]), ALL, gamma=GAMMA, alpha=ALPHA, bootstrap=3, seed=SEED, draw=FRESH)
    _install(c)
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=3)
    _, got = TQ._q_steps(env, 2, 33, "value")
    q_got = _snap(env, q_next=False)
    clean = TQ._env(c["feeder"], c["B"], c["ep"])
    try:
        _install(dict(c, env=clean))
        clean.reset(seed=3)
        rollout_device(clean, c["T"], reset=False, actions=c["data"]["actions"])
        P.evaluate_rollout(clean, gamma=GAMMA, lam=0.95, bootstrap=3)
        P.evaluate_rollout_q(clean, gamma=GAMMA, bootstrap=3)
        OnPolicyBatches(clean, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=TQ.FIELDS).prepare()
        _, want = TQ._q_steps(clean, 2, 33, "value")
        for k, x in _snap(clean, q_next=False).items():
            assert _same(x, q_got[k]), k
        for a, b in zip(got, want):
            for w in range(2):
                for k in ("params", "grads", "m", "v"):
                    assert _same(a[w][k], b[w][k]), (w, k)
    finally:
        clean.close()


def test_every_refusal_leaves_every_arrays_bits(prepared):
    c = prepared("ieee13-relu")
    env, mask = c["env"], 3
    h = env.handle
    _install(c)
    _evaluate_all(env, mask, STALE)
    before = _snap(env)
    batch = _dev(np.arange(33))
    cfg = lambda **kw: _lib.refresh_config(**dict(dict(groups=15, gamma=GAMMA, alpha=ALPHA, bootstrap_mask=mask, seed=SEED, draw=FRESH), **kw))
    for bad, text in ((cfg(struct_size=64), "struct_size"), (cfg(groups=0), "groups"), (cfg(groups=16), "groups"), (cfg(groups=31), "groups"),
                      (cfg(bootstrap_mask=4), "mask"), (cfg(bootstrap_mask=-1), "mask"), (cfg(gamma=math.nan), "gamma"), (cfg(gamma=math.inf), "gamma"),
                      (cfg(reward_shift=math.inf), "gamma"), (cfg(reward_scale=math.nan), "gamma"), (cfg(alpha=math.nan), "alpha"), (cfg(alpha=-0.5), "alpha"),
                      (cfg(alpha=math.inf), "alpha")):
        TQ._refused(lambda: h.learner_refresh(batch, bad), I, text)
    two = cfg()
    two.stochastic = 2
    TQ._refused(lambda: h.learner_refresh(batch, two), I, "stochastic")
    for n in (0, -1, (1 << 24) + 1):
        TQ._refused(lambda: h.learner_refresh(batch, cfg(), n=n), I, "outside 1 .. 2^24")
    TQ._refused(lambda: h.learner_refresh({}, cfg(), n=33), I, "no indices")
    # the evaluation a group replaces rows of ran under another mask
    TQ._refused(lambda: h.learner_refresh(batch, cfg(groups=1, bootstrap_mask=1)), S, "bootstrap_mask")
    # a network a group needs is not installed
    env.set_value(None)
    for g in (_lib.GS_REFRESH_TD_VALUE, _lib.GS_REFRESH_Q_ADV, 15):
        TQ._refused(lambda: h.learner_refresh(batch, cfg(groups=g)), S, "gs_value_mlp_set")
    h.learner_refresh(batch, cfg(groups=_lib.GS_REFRESH_Q_TARGET))      # (needs no value network; unchanged images: the same bits)
    env.set_value(c["val"])
    after = _snap(env)
    for k, x in before.items():
        assert _same(x, after[k]), k
    # the evaluations are not current: a fresh handle, step by step
    fresh = TQ._env(c["feeder"], c["B"], c["ep"])
    try:
        hf = fresh.handle
        fresh.set_policy(c["pol"], stochastic=True)
        fresh.set_q(0, c["qs"][0])
        TQ._refused(lambda: hf.learner_refresh(batch, cfg()), S, "no rollout")
        fresh.set_q(0, None)
        fresh.reset(seed=3)
        rollout_device(fresh, c["T"], reset=False, actions=c["data"]["actions"])
        TQ._refused(lambda: hf.learner_refresh(batch, cfg()), S, "before gs_q_mlp_set")
        for w in range(2):
            fresh.set_q(w, c["qs"][w])
        TQ._refused(lambda: hf.learner_refresh(batch, cfg(groups=1)), S, "gs_rollout_evaluate_q_next, which has not run")
        for g in (2, 4, 8):
            TQ._refused(lambda: hf.learner_refresh(batch, cfg(groups=g)), S, "gs_rollout_evaluate_q, which has not run")
        fresh.set_value(c["val"])
        P.evaluate_rollout(fresh, gamma=GAMMA, lam=0.95, bootstrap=mask)
        P.evaluate_rollout_q(fresh, gamma=GAMMA, bootstrap=mask)
        TQ._refused(lambda: hf.learner_refresh(batch, cfg()), S, "gs_rollout_evaluate_q_next, which has not run")
        hf.learner_refresh(batch, cfg(groups=14))
        plain = P.MLPPolicy(*TQ._layers([fresh.obs_dim, 64, fresh.action_dim], 1), activation="relu", head="tanh", compute="float32")
        fresh.set_policy(plain)
        TQ._refused(lambda: hf.learner_refresh(batch, cfg(groups=1)), S, "GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH")
        fresh.set_policy(c["pol"], stochastic=True)
        P.evaluate_rollout_q_next(fresh, gamma=GAMMA, alpha=ALPHA, bootstrap=mask, seed=SEED, draw=STALE)
        hf.learner_refresh(batch, cfg())
        # a further rollout makes both evaluations stale
        rollout_device(fresh, c["T"], reset=False, actions=c["data"]["actions"])
        TQ._refused(lambda: hf.learner_refresh(batch, cfg(groups=1)), S, "has not run")
        TQ._refused(lambda: hf.learner_refresh(batch, cfg(groups=2)), S, "has not run")
    finally:
        fresh.close()
