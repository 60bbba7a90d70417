"""GPU: the per-minibatch refresh (``gs_learner_refresh``: the five kernels of kernels_refresh.hip, the terminal map and the scratch
blocks of abi_refresh.hip; DESIGN.md section 27 "The edges") at its chunk, mask, clamp and buffer edges -- the table of
tests/refresh_cases.py, held to its rules on the host by tests/test_refresh_cases_static.py.  What the lists, the masks 0 and 3 and
the one rollout per handle of tests/test_gpu_refresh.py (imported, not edited) cannot see:

1. chunks and waves    lists of three and four chunks of ``gs_k_refresh_terms``, waves with every lane set, a compacted list longer
                       than the rollout's terminal list, n = 256, 257, 512, 513
2. single masks        masks 1 and 2 alone: ``done[j] & mask`` filters, a done row WITHOUT a pair lies between two rows with one;
                       a list that is empty while the terminal path is on
3. the clamp           indices below 0 and at or above N, down to -2^31 and up to 2^31 - 1
4. capacity, the map   T < T_cap, release and regrow, a second rollout whose episodes end at other steps
5. the arithmetic      reward shift and scale, the deterministic head, alpha = 0, one twin alone
6. n                   a growing and a shrinking n on one handle (``r.q + w * n`` follows n)

The oracle and the comparison are tests/test_gpu_refresh.py's ``_check`` and ``_restatements`` (``_restate`` below passes the
arguments the latter fixes -- draw, shift and scale, alpha, the head -- and adds the other groups' restatements): at the rows of a
list and the terminal entries reached from it the bits of a full ``evaluate_rollout_q_next`` / ``evaluate_rollout_q`` under the same
config and images, everywhere else the bits downloaded just before the refresh; ``td_target``, ``td_value``, the minima, ``q_adv``
and ``term_value`` bit-equal to ``td_policy_np`` / ``td_target_np`` fed the device's arrays; the noise within the project's 1e-9 of
``q_next_noise_np``.  No bound is new and none is computed from the device.

No check is vacuous, by construction: before a refresh the arrays are left under ANOTHER draw, the plain settings and OTHER images
-- a value network of another seed (``set_value`` leaves the evaluations current) and the twins as they were before one Q step per
twin and ``update_targets(0.5)``.  (Installing a twin marks both evaluations as not current, and a refresh is refused then: the
twins move the way tests/test_gpu_refresh.py moves them.)  The full evaluation the refresh is compared with runs on the SAME handle
right after it, under the images the refresh saw.  Networks are (64, 64) relu throughout."""
import ctypes as C

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import pathwise_tanh_np
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, q_next_noise_np, refresh_rows_np, refresh_targets, rollout_device, td_policy_np, td_target_np
from tests import refresh_cases as R
from tests import test_gpu_q_next as TQ
from tests import test_gpu_q_next_shapes as QS
from tests import test_gpu_refresh as TR

pytestmark = pytest.mark.gpu

GAMMA, ALPHA, SEED, STALE, FRESH, ALL = TR.GAMMA, TR.ALPHA, TR.SEED, TR.STALE, TR.FRESH, TR.ALL
_same, _snap = TQ._same, TR._snap
_HANDLES, _BUFFERS = {}, []


@pytest.fixture(scope="module")
def handle():
    """``handle(name, recipe)``: an environment of the recipe with the networks, made once and closed with the module"""
    def get(name, recipe=R.BASE):
        if name not in _HANDLES:
            _HANDLES[name] = _make(recipe)
        return _HANDLES[name]
    yield get
    for c in _HANDLES.values():
        c["env"].close()
    _HANDLES.clear()
    hip = _lib._hip_runtime()
    for p in _BUFFERS:
        hip.hipFree(p)
    _BUFFERS.clear()


def _make(recipe):
    env = QS._env(recipe.feeder, recipe.B, recipe.episode_length, recipe.limits)
    pol, val, qs = TQ._networks(recipe.feeder, env.obs_dim, env.action_dim, [64, 64], "relu")
    mean, std = TQ._normalisation(recipe.feeder)
    other = P.MLPValue(*TQ._layers([env.obs_dim, 64, 1], 3), activation="relu", obs_mean=mean, obs_std=std)
    return dict(env=env, pol=pol, val=val, qs=qs, other_val=other, feeder=recipe.feeder, B=recipe.B, ep=recipe.episode_length, recipe=recipe)


def _dev(idx):
    """a batch that holds nothing but these indices, in device memory of the test's own"""
    a = np.ascontiguousarray(idx, dtype=np.int32)
    assert np.array_equal(a, idx)
    hip = _lib._hip_runtime()
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 4))) == 0 and p.value
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0      # hipMemcpyHostToDevice
    _BUFFERS.append(p)
    return dict(indices=_lib.DeviceArray(p.value, a.shape, "<i4"))


def _evaluate_all(env, mask, draw, alpha=ALPHA, stochastic=True, shift=0.0, scale=1.0):
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=mask)
    P.evaluate_rollout_q(env, gamma=GAMMA, bootstrap=mask, reward_shift=shift, reward_scale=scale)
    P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=alpha, bootstrap=mask, stochastic=stochastic, seed=SEED, draw=draw, reward_shift=shift, reward_scale=scale)


def _begin(c, data=None, twins=(0, 1)):
    """the rollout ``data`` (the recipe's own when None and none is there yet) becomes the handle's current one: the networks as
    first installed (``twins``: the others are taken out), the minibatches prepared, a Q learner on the installed twins"""
    env = c["env"]
    if data is None and "data" not in c:
        data = QS._collect(env, c["recipe"].T)
    if data is not None:
        c["data"], c["T"] = data, data["rewards"].shape[0]
    TQ._install(c, twins=twins)
    for w in range(2):
        if w not in twins:
            env.set_q(w, None)
    c["twins"] = tuple(twins)
    P.evaluate_rollout(env, gamma=GAMMA, lam=0.95, bootstrap=3)
    OnPolicyBatches(env, c["B"] * c["T"], policy=c["pol"], adv_norm="none", seed=5, fields=TQ.FIELDS).prepare()
    c["learner"] = P.DeviceLearner(env, nets=tuple(f"q{w + 1}" for w in twins), **TQ.HYPER)
    c["steps"] = 0
    return c


def _collected(c):
    """a shared handle with its recipe's rollout collected and both twins installed"""
    if "data" not in c or c["twins"] != (0, 1):
        _begin(c)
    return c


def _move_twins(c):
    """one Q step per installed twin and a target update: both images of every twin are other bits than before"""
    learner, h = c["learner"], c["env"].handle
    learner.step(h.onpolicy_batch(5, c["steps"], 0, min(64, c["T"] * c["B"])))
    learner.update_targets(0.5)
    c["steps"] += 1


def _restate(c, idx, mask, groups, after, own, pairs, values, alpha=ALPHA, stochastic=True, shift=0.0, scale=1.0):
    """tests/test_gpu_refresh.py's ``_restatements`` under the arguments it fixes, and the other groups' restatements: every signal a
    step reads, at the refreshed rows, against the NumPy restatements fed the device's arrays"""
    d, T, B, twins = c["data"], c["T"], c["B"], c["twins"]
    A, N = c["env"].action_dim, c["T"] * c["B"]
    at = lambda x: np.ascontiguousarray(x.reshape(N, -1)[own])
    least = lambda q0, q1: np.fmin(q0, q1) if len(twins) == 2 else (q0, q1)[twins[0]]
    if "td_policy" in groups and (alpha, stochastic, shift, scale, twins) == (ALPHA, True, 0.0, 1.0, (0, 1)):
        TR._restatements(c, idx, mask, after, own, pairs)
    elif "td_policy" in groups:            # the same statements under the arguments it fixes
        e = pairs[:, 1]
        ti = d["terminal_index"][e]
        if stochastic:
            assert TQ._err(at(after["next_noise"]), q_next_noise_np(SEED, FRESH, own, A)) <= 1e-9 and np.abs(at(after["next_noise"])).max() > 0.0
            if len(e):
                assert TQ._err(after["term_noise"][e], q_next_noise_np(SEED, FRESH, ti[:, 0].astype(np.int64) * B + ti[:, 1], A, terminal=True)) <= 1e-9
        else:
            for eps, pre, act in ((at(after["next_noise"]), at(after["next_pre_head"]), at(after["next_actions"])),
                                  (after["term_noise"][e], after["term_pre_head"][e], after["term_actions"][e])):
                assert not eps.any() and not np.signbit(eps).any()                      # +0.0
                assert _same(act, pathwise_tanh_np(pre[:, :A].astype(np.float64)))
        want = td_policy_np(d["rewards"], after["next_log_probs"], after["q_next_min"], d["terminals"], after["term_q_min"], d["terminal_index"], GAMMA, alpha, mask,
                            shift, scale, terminal_log_probs=after["term_log_probs"])
        assert _same(at(after["td_target"]), at(want))
        assert _same(at(after["q_next_min"]), at(least(after["q_next0"], after["q_next1"])))
        assert _same(after["term_q_min"][e], least(after["term_q0"], after["term_q1"])[e])
        assert _same(after["term_value"][e], (after["term_q_min"] - alpha * after["term_log_probs"])[e])
    if "td_value" in groups:
        want = td_target_np(d["rewards"], values["values"], d["terminals"], values["terminal_values"], d["terminal_index"], GAMMA, mask, shift, scale)
        assert _same(at(after["td_value"]), at(want))
    if "q_target" in groups:
        assert _same(at(after["q_min_target"]), at(least(after["q_target0"], after["q_target1"])))
    if "q_adv" in groups:
        assert _same(at(after["q_min_online"]), at(least(after["q_online0"], after["q_online1"])))
        assert _same(at(after["q_adv"]), at(after["q_min_online"] - values["values"][:T]))
    for w in range(2):                        # a twin that is not installed: its arrays are not there, before and after
        if w not in twins:
            for k in (f"q_next{w}", f"term_q{w}", f"q_online{w}", f"q_target{w}"):
                assert np.isnan(after[k]).all(), k


def _refresh(c, idx, mask, groups=ALL, tag="", constant=(), **variant):
    """The common check.  The arrays are left under draw STALE, the plain settings, another value network and the twins' images
    before a step; ``idx`` is refreshed under draw FRESH and ``variant``; the full evaluations under FRESH and ``variant`` then run on
    the same handle.  Returns (own, pairs, before, after, fresh)."""
    env = c["env"]
    env.set_value(c["other_val"])
    _evaluate_all(env, mask, STALE)
    env.set_value(c["val"])
    _move_twins(c)
    before = _snap(env)
    kw = dict(alpha=variant.get("alpha", ALPHA), stochastic=variant.get("stochastic", True))
    rs = dict(reward_shift=variant.get("shift", 0.0), reward_scale=variant.get("scale", 1.0))
    refresh_targets(env, _dev(idx), groups, gamma=GAMMA, bootstrap=mask, seed=SEED, draw=FRESH, **kw, **rs)
    after = _snap(env)
    _evaluate_all(env, mask, FRESH, **variant)
    fresh = _snap(env)
    values = env.handle.rollout_onpolicy_download(("values", "terminal_values"))
    own, pairs = TR._check(c, idx, mask, groups, before, after, fresh, tag=tag, constant=constant)
    _restate(c, idx, mask, groups, after, own, pairs, values, **variant)
    return own, pairs, before, after, fresh


def _base(handle):
    c = _collected(handle("base"))
    flags, ti = c["data"]["terminals"], c["data"]["terminal_index"]
    assert _same(flags, R.base_flags()), "the base's terminal transitions are 65 .. 129 and 195 .. 259, all at the time limit"
    assert len(ti) == R.TERM_CAP and np.array_equal(np.sort(ti[:, 0].astype(np.int64) * c["B"] + ti[:, 1]), np.nonzero(flags.reshape(-1))[0])
    return c


# ---- 1. chunks and waves ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.BASE_LISTS))
def test_chunks_and_waves(handle, name):
    """All four groups under mask 3 over every list of the table.  The length of the compacted list is seen through the entries
    that change: exactly those of ``refresh_rows_np``'s pairs, each to the full evaluation's bits (``_check``), and no entry a pair
    names keeps its stale noise."""
    c = _base(handle)
    idx = R.BASE_LISTS[name]
    own, pairs, before, after, fresh = _refresh(c, idx, 3, ALL, tag=name)
    model = R.refresh_terms_np(idx, c["data"]["terminals"], R.terminal_map_np(c["data"]["terminal_index"], c["T"], c["B"]), 3)
    assert model.count == len(pairs) > 0 and np.array_equal(model.ie[:model.count], pairs)
    hit = np.zeros(R.TERM_CAP, dtype=bool)
    hit[pairs[:, 1]] = True
    changed = (after["term_noise"] != before["term_noise"]).any(axis=1)
    assert np.array_equal(changed, hit), "the entries that change are the list's"
    if name in ("all3", "perm3", "terminal", "terminal4"):
        assert hit.all() and (after["term_value"] != before["term_value"]).all() and (after["term_q_min"] != before["term_q_min"]).all()
    if name == "terminal4":
        assert len(pairs) == len(idx) == 520 and np.array_equal(pairs[:, 0], np.arange(520))
        for k in TR.TERM_KEYS:
            assert _same(after[k], fresh[k]), k


# ---- 2. single masks --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [1, 2])
def test_single_masks(handle, mask):
    """The 185-row dataset under mask 1 and under mask 2 alone, ``td_policy`` and ``td_value`` over ``all`` and ``twice``: on each
    list some done row WITHOUT a pair lies between two rows with one (asserted on the downloaded flags), and its targets are the
    reward term alone."""
    c = _collected(handle("small", R.SMALL))
    d, T, B = c["data"], c["T"], c["B"]
    flags = d["terminals"].reshape(-1)
    assert ((flags & mask) != 0).any() and ((flags != 0) & ((flags & mask) == 0)).any(), "the mask filters"
    for tag, idx in R.small_lists().items():
        own, pairs, before, after, fresh = _refresh(c, idx, mask, ("td_policy", "td_value"), tag=(tag, mask))
        lone = R.lone_done_row_between_pairs(idx, d["terminals"], d["terminal_index"], T, B, mask)
        assert len(lone) and 0 < len(pairs) < len(refresh_rows_np(idx, T, B, d["terminals"], d["terminal_index"], 3)[2])
        j = own[lone]
        reward_alone = d["rewards"].reshape(-1)[j] + GAMMA * 0.0
        assert _same(after["td_target"].reshape(-1)[j], reward_alone) and _same(after["td_value"].reshape(-1)[j], reward_alone)


def test_an_empty_list_while_the_terminal_path_is_on(handle):
    """The base under mask 2: every done row is a time limit, so the compacted list is empty (``count`` = 0 with the terminal
    launches queued), no terminal entry changes, and the targets at done rows are the reward term alone."""
    c = _base(handle)
    d = c["data"]
    done = d["terminals"].reshape(-1) != 0
    for name in ("terminal", "n257"):
        idx = R.BASE_LISTS[name]
        # (on the terminal-only list every td_value is r' alone, whatever the value network: asserted to be the stale bits)
        own, pairs, before, after, fresh = _refresh(c, idx, 2, ("td_policy", "td_value"), tag=(name, 2), constant=("td_value",) if name == "terminal" else ())
        assert len(pairs) == 0 and done[own].any()
        for k in TR.TERM_KEYS:
            assert _same(after[k], before[k]), k
        j = own[done[own]]
        reward_alone = d["rewards"].reshape(-1)[j] + GAMMA * 0.0
        assert _same(after["td_target"].reshape(-1)[j], reward_alone) and _same(after["td_value"].reshape(-1)[j], reward_alone)


# ---- 3. the clamp -----------------------------------------------------------------------------------------------------------------------

def _edges_reach(c, own, pairs, after, fresh, N):
    idx = R.BASE_LISTS["edges"]
    assert np.array_equal(own, R.clamp(idx, N)) and list(own[:7]) == [0, 0, 0] + [min(259, N - 1)] * 4
    for k in ("td_target", "td_value", "q_min_target", "q_adv", "next_log_probs"):
        for row in (0, N - 1):
            assert _same(after[k].reshape(-1)[row:row + 1], fresh[k].reshape(-1)[row:row + 1]), (k, row)


def test_the_clamp(handle):
    """``edges`` on the base: -1, -2^31 and 0 land on row 0; 259, 260, 265 and 2^31 - 1 on row 259, which is terminal, so the clamped
    index reaches the terminal path: rows 0 and 259 and the entry of (3, 64) hold the fresh bits.  The same list under T < T_cap,
    where index N must land on row N - 1, runs in the capacity test below."""
    c = _base(handle)
    own, pairs, before, after, fresh = _refresh(c, R.BASE_LISTS["edges"], 3, ALL, tag="edges")
    _edges_reach(c, own, pairs, after, fresh, 260)
    ti = c["data"]["terminal_index"]
    e = int(np.nonzero((ti[:, 0] == 3) & (ti[:, 1] == 64))[0][0])
    assert [tuple(p) for p in pairs[:4]] == [(3, e), (4, e), (5, e), (6, e)]
    for k in TR.TERM_KEYS:
        assert _same(after[k][e:e + 1], fresh[k][e:e + 1]), k
    assert not np.array_equal(after["term_noise"][e], before["term_noise"][e]) and after["term_value"][e] != before["term_value"][e]


# ---- 4. capacity and the map's key ------------------------------------------------------------------------------------------------------

def _stage(c, data, lists, tag):
    """a further rollout on the handle, evaluated and refreshed; afterwards one more evaluation under another draw, so that what
    this rollout leaves behind is not what the next one computes"""
    _begin(c, data)
    out = [_refresh(c, idx, 3, ALL, tag=(tag, name)) for name, idx in lists]
    _evaluate_all(c["env"], 3, STALE + 1)
    return out


def test_capacity_and_the_maps_key(handle):
    """The arrays are laid out by ``T_cap * B``, the clamp takes ``T * B``, and the terminal map is refilled once per rollout.
    Handle one: T = 4, then T = 1 (T < T_cap, no terminal entry; indices 65 and 259 land on row 64), then T = 4 again.  Handle two:
    T = 1 first, then T = 4 (release and regrow).  Handle three: T = 3 from a reset, then 4 steps WITHOUT a reset, whose episodes
    end at other steps (asserted): a map kept from the first rollout would reach the wrong entries."""
    all3, edges = ("all3", R.BASE_LISTS["all3"]), ("edges", R.BASE_LISTS["edges"])
    one = ("rows + [65, 259]", np.concatenate([np.arange(65), [65, 259]]))
    handles = [_make(R.BASE) for _ in range(3)]
    try:
        a, b, c = handles
        _stage(a, QS._collect(a["env"], 4), [all3], "a: T4")
        short = _stage(a, QS._collect(a["env"], 1), [one, edges], "a: T1 < T_cap")
        assert a["T"] == 1 and len(a["data"]["terminal_index"]) == 0
        own, pairs, _, after, fresh = short[0]
        assert list(own[-2:]) == [64, 64] and len(pairs) == 0
        own, pairs, _, after, fresh = short[1]
        _edges_reach(a, own, pairs, after, fresh, 65)
        assert (own[3:7] == 64).all() and len(pairs) == 0
        _stage(a, QS._collect(a["env"], 4), [all3], "a: T4 again")
        _stage(b, QS._collect(b["env"], 1), [one], "b: T1")
        _stage(b, QS._collect(b["env"], 4), [all3], "b: T4 regrown")
        first = QS._collect(c["env"], 3)
        _stage(c, first, [("all", np.arange(195))], "c: T3")
        rollout_device(c["env"], 4, seed=8, reset=False)
        second = TQ._rollout_arrays(c["env"])
        ends = lambda d: sorted((int(t), int(b)) for t, b in d["terminal_index"])
        assert len(ends(first)) and len(ends(second)) and {t for t, _ in ends(first)}.isdisjoint({t for t, _ in ends(second)}), "episodes end at other steps"
        own, pairs, *_ = _stage(c, second, [all3], "c: T4 without a reset")[0]
        assert len(pairs) == 3 * len(second["terminal_index"])
    finally:
        for x in handles:
            x["env"].close()


# ---- 5. the arithmetic the refresh kernels restate -----------------------------------------------------------------------------------

VARIANTS = {"shift-scale": (dict(shift=0.5, scale=0.25), ("td_policy", "td_value")), "deterministic": (dict(stochastic=False), ("td_policy",)),
            "alpha-0": (dict(alpha=0.0), ("td_policy",))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restated_arithmetic(handle, variant):
    """One variant at a time on the base under mask 3, lists ``n257`` and ``terminal``; evaluated and refreshed under the variant,
    the stale arrays left under the plain settings."""
    c = _base(handle)
    kw, groups = VARIANTS[variant]
    for name in ("n257", "terminal"):
        own, pairs, before, after, fresh = _refresh(c, R.BASE_LISTS[name], 3, groups, tag=(variant, name), **kw)
        assert len(pairs) > 0
        if variant == "shift-scale":          # the targets are not those of the plain settings on the same arrays
            plain = td_policy_np(c["data"]["rewards"], after["next_log_probs"], after["q_next_min"], c["data"]["terminals"], after["term_q_min"],
                                 c["data"]["terminal_index"], GAMMA, ALPHA, 3, terminal_log_probs=after["term_log_probs"])
            assert (after["td_target"].reshape(-1)[own] != plain.reshape(-1)[own]).all()


@pytest.mark.parametrize("w", [0, 1])
def test_one_twin_alone(handle, w):
    """Twin ``w`` alone, all four groups: the NULL-twin branch of three kernels and ``r.q + w * n`` for w = 1 alone.  The minimum is
    the present twin's value; the absent twin's arrays are not there before or after (the download leaves them NaN)."""
    c = _base(handle)
    _begin(c, c["data"], twins=(w,))
    try:
        for name in ("n257", "terminal"):
            own, pairs, before, after, fresh = _refresh(c, R.BASE_LISTS[name], 3, ALL, tag=(f"twin {w}", name))
            assert c["env"].handle.rollout_q_next_arrays()["installed"] == (w,) and c["env"].handle.rollout_q_arrays()["installed"] == (w,)
            for least, twin in (("q_next_min", "q_next"), ("term_q_min", "term_q"), ("q_min_online", "q_online"), ("q_min_target", "q_target")):
                assert _same(after[least], after[f"{twin}{w}"]) and np.isfinite(after[f"{twin}{w}"]).all(), least
                assert np.isnan(before[f"{twin}{1 - w}"]).all() and np.isnan(after[f"{twin}{1 - w}"]).all(), twin
    finally:
        _begin(c, c["data"])


# ---- 6. a growing and a shrinking n -------------------------------------------------------------------------------------------------

def test_a_growing_and_a_shrinking_n_on_one_handle(handle):
    """n = 513 first (the scratch is made), then 1, then 257 (in place), then 780 (regrown): the second twin's block lies at ``r.q +
    n``, wherever the capacity ends"""
    c = _make(R.BASE)
    try:
        _begin(c)
        for name, idx in (("n513", R.BASE_LISTS["n513"]), ("n=1", R.BASE_LISTS["perm3"][:1]), ("n257", R.BASE_LISTS["n257"]), ("all3", R.BASE_LISTS["all3"])):
            _refresh(c, idx, 3, ALL, tag=name)
    finally:
        c["env"].close()
